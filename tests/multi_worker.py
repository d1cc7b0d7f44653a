"""TEST worker (tests/test_gpu_multi.py): one rank, launched by ftrun, of a run of the torch
binding's Comm.allreduce_multi.  The rank's dense float32 vector in_<rank>.bin is cut into one
torch tensor per entry of MULTI_COUNTS on the rank's GPU; call 0 reduces the list in place with
the default schedule, call 1 out of place with algo="rd", call 2 a list of packed FLOAT_INT pairs
(dtype=) with MAXLOC.  Writes out_<rank>_<k>.bin (the results, concatenated) and
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
    a = torch.from_numpy(np.fromfile(os.path.join(d, f"in_{rank}.bin"), dtype=np.float32))
    cuts = list(torch.split(a, counts))

    def finish(k, rc, outs, untouched):
        torch.cuda.synchronize()
        flat = torch.cat([o.reshape(-1).cpu() for o in outs]) if outs else torch.zeros(0)
        flat.numpy().tofile(os.path.join(d, f"out_{rank}_{k}.bin"))
        with open(os.path.join(d, f"status_{rank}_{k}.txt"), "w") as f:
            f.write(f"{rc} {comm.last_stats().coalesced} {int(untouched)}\n")

    ts = [c.cuda() for c in cuts]
    rc = comm.allreduce_multi(ts)  # in place, Rabenseifner
    finish(0, rc, ts, True)
    ts = [c.cuda() for c in cuts]
    outs = [torch.full_like(t, float("nan")) for t in ts]
    rc = comm.allreduce_multi(ts, out=outs, op=ftar.MAX, algo="rd")
    finish(1, rc, outs, all(torch.equal(t.cpu(), c) for t, c in zip(ts, cuts)))
    # pairs: the value and, as the index, rank * total + position (distinct over the job)
    base, ps = 0, []
    for c in cuts:
        idx = torch.arange(base, base + c.numel(), dtype=torch.int64) + rank * a.numel()
        ps.append(ftar.pack_pairs(c.cuda(), idx.cuda(), ftar.FLOAT_INT))
        base += c.numel()
    rc = comm.allreduce_multi(ps, op=ftar.MAXLOC, dtype=ftar.FLOAT_INT)
    finish(2, rc, [p.view(torch.float32) for p in ps], True)
    comm.finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
