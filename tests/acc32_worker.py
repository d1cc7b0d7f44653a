"""TEST worker (tests/test_gpu_acc32.py): one rank, launched by ftrun, of a run of the torch
binding's Comm.allreduce_multi_acc32.  The rank's dense vectors in_<rank>_<k>.bin (uint16 bit
patterns) are cut into one torch tensor per entry of MULTI_COUNTS on the rank's GPU; call 0 reduces
a bfloat16 list in place with SUM, scale 0.5 and the default schedule, call 1 a float16 list out of
place with MAX and algo="rd".  Writes out_<rank>_<k>.bin (the results, concatenated) and
status_<rank>_<k>.txt: "rc coalesced inputs_untouched".

env: FTAR_PROBE_DIR, MULTI_COUNTS="1,3,0,5" (set by the test), FTAR_RANK / FTAR_DEVICE (ftrun)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    d = os.environ["FTAR_PROBE_DIR"]
    rank = int(os.environ["FTAR_RANK"])
    counts = [int(c) for c in os.environ["MULTI_COUNTS"].split(",")]
    torch.cuda.set_device(int(os.environ.get("FTAR_DEVICE", "0")))
    spec = importlib.util.spec_from_file_location("ftar_amd", os.path.join(ROOT, "fault-tolerant_amd", "__init__.py"))
    ftar = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ftar)
    comm = ftar.Comm.from_env()

    def cuts(k, dtype):
        a = torch.from_numpy(np.fromfile(os.path.join(d, f"in_{rank}_{k}.bin"), dtype=np.int16)).view(dtype)
        return list(torch.split(a, counts))

    def finish(k, rc, outs, untouched):
        torch.cuda.synchronize()
        flat = torch.cat([o.reshape(-1).cpu() for o in outs])
        flat.view(torch.int16).numpy().tofile(os.path.join(d, f"out_{rank}_{k}.bin"))
        with open(os.path.join(d, f"status_{rank}_{k}.txt"), "w") as f:
            f.write(f"{rc} {comm.last_stats().coalesced} {int(untouched)}\n")

    ts = [c.cuda() for c in cuts(0, torch.bfloat16)]
    rc = comm.allreduce_multi_acc32(ts, scale=0.5)  # in place, Rabenseifner, SUM
    finish(0, rc, ts, True)
    host = cuts(1, torch.float16)
    ts = [c.cuda() for c in host]
    outs = [torch.full_like(t, float("nan")) for t in ts]
    rc = comm.allreduce_multi_acc32(ts, out=outs, op=ftar.MAX, algo="rd")
    finish(1, rc, outs, all(torch.equal(t.cpu().view(torch.int16), c.view(torch.int16)) for t, c in zip(ts, host)))
    comm.finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
