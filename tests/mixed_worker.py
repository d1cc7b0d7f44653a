"""TEST worker (tests/test_gpu_mixed.py): one rank, launched by ftrun, of a run of the torch
binding's Comm.allreduce_multi_mixed.  The rank's list bytes in_<rank>_<k>.bin (entry after entry,
each in its own type) are cut into one torch tensor per entry of MULTI_COUNTS / MIXED_TYPES on the
rank's GPU; call 0 reduces the list in place with SUM, scale 0.5 and the default schedule, call 1
out of place with MAX and algo="rd".  Writes out_<rank>_<k>.bin (the results' bytes, concatenated)
and status_<rank>_<k>.txt: "rc coalesced inputs_untouched".

env: FTAR_PROBE_DIR, MULTI_COUNTS="1,3,0,5", MIXED_TYPES="17,1,16,1" (set by the test),
     FTAR_RANK / FTAR_DEVICE (ftrun)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {1: (torch.float32, np.float32, 4), 16: (torch.float16, np.int16, 2), 17: (torch.bfloat16, np.int16, 2)}


def main():
    d = os.environ["FTAR_PROBE_DIR"]
    rank = int(os.environ["FTAR_RANK"])
    counts = [int(c) for c in os.environ["MULTI_COUNTS"].split(",")]
    types = [int(t) for t in os.environ["MIXED_TYPES"].split(",")]
    torch.cuda.set_device(int(os.environ.get("FTAR_DEVICE", "0")))
    spec = importlib.util.spec_from_file_location("ftar_amd", os.path.join(ROOT, "fault-tolerant_amd", "__init__.py"))
    ftar = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ftar)
    comm = ftar.Comm.from_env()

    def cuts(k):
        raw = np.fromfile(os.path.join(d, f"in_{rank}_{k}.bin"), dtype=np.uint8)
        out, b = [], 0
        for c, t in zip(counts, types):
            td, nd, es = DT[t]
            out.append(torch.from_numpy(raw[b:b + c * es].view(nd).copy()).view(td))
            b += c * es
        return out

    def raw_of(ts):
        return np.concatenate([t.reshape(-1).cpu().view(torch.uint8).numpy() if t.numel() else np.empty(0, np.uint8) for t in ts])

    def finish(k, rc, outs, untouched):
        torch.cuda.synchronize()
        raw_of(outs).tofile(os.path.join(d, f"out_{rank}_{k}.bin"))
        with open(os.path.join(d, f"status_{rank}_{k}.txt"), "w") as f:
            f.write(f"{rc} {comm.last_stats().coalesced} {int(untouched)}\n")

    ts = [c.cuda() for c in cuts(0)]
    rc = comm.allreduce_multi_mixed(ts, scale=0.5)  # in place, Rabenseifner, SUM
    finish(0, rc, ts, True)
    host = cuts(1)
    ts = [c.cuda() for c in host]
    outs = [torch.full_like(t, float("nan")) for t in ts]
    rc = comm.allreduce_multi_mixed(ts, out=outs, op=ftar.MAX, algo="rd")
    finish(1, rc, outs, np.array_equal(raw_of(ts), raw_of(host)))
    comm.finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
