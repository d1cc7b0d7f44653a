"""TEST worker for the pair types (tests/test_gpu_pair.py): every GPU action of those tests
happens in a process of this program, never in the pytest process.

Like half_worker.py it binds the product library through the package and takes device memory
from the HIP runtime the library is linked with (no torch).  Buffers are raw bytes: windows are
given as byte offsets, counts in elements of the case's pair type.

env: FTAR_PROBE_DIR (the job's directory), PAIR_MODE=

  local   run directly.  cases.json lists {"dtype", "op", "n", "off_in", "off_io", "variant"};
          case i reads the whole buffers lin_i.bin and lio_i.bin, reduces n elements at the two
          byte offsets with ftar_set_reduce_variant(variant) and writes the whole in-out buffer
          to lout_i.bin.  status.txt: one line "rc in_untouched" per case.

  sched   one rank under ftrun.  calls.json lists {"dtype", "algo": "raben"|"rd", "op",
          "inplace", "offset", "host"}; call k reads in_<rank>_<k>.bin, puts it at byte `offset`
          of a guarded buffer (device memory, or pageable host memory for the *_host entry
          points), runs the Allreduce and writes out_<rank>_<k>.bin and status_<rank>_<k>.txt:
          "rc comm_size_after recoveries intact" (intact: the guards around both windows, and
          the send window unless in place, still hold what was put there).
"""
import json
import os
import sys

import numpy as np

from half_worker import Hip, load_package

DTYPES = {"float_int": (32, 8), "2int": (33, 8), "double_int": (34, 16)}  # name: (ftar_dtype, bytes)
GUARD_S, GUARD_R, PAD = 0x5A, 0xEE, 32


def run_local(ftar, hip, d):
    hip.set_device(int(os.environ.get("FTAR_DEVICE", "0")))
    cases = json.load(open(os.path.join(d, "cases.json")))
    lines = []
    for i, c in enumerate(cases):
        dt, es = DTYPES[c["dtype"]]
        a = np.fromfile(os.path.join(d, f"lin_{i}.bin"), dtype=np.uint8)
        b = np.fromfile(os.path.join(d, f"lio_{i}.bin"), dtype=np.uint8)
        assert c["off_in"] + c["n"] * es <= a.size and c["off_io"] + c["n"] * es <= b.size, c  # inside the buffers
        ftar.set_reduce_variant(c["variant"])
        pa, pb = hip.upload(a), hip.upload(b)
        rc = ftar.lib().ftar_reduce_local(pa + c["off_in"], pb + c["off_io"], c["n"], dt, c["op"], None)
        out = hip.download(pb, b)
        same = bool(np.array_equal(hip.download(pa, a), a))
        out.tofile(os.path.join(d, f"lout_{i}.bin"))
        hip.free(pa)
        hip.free(pb)
        lines.append(f"{rc} {int(same)}\n")
    with open(os.path.join(d, "status.txt"), "w") as f:
        f.writelines(lines)
    return 0


def run_sched(ftar, hip, d):
    rank = int(os.environ["FTAR_RANK"])
    comm = ftar.Comm.from_env()
    hip.set_device(comm.device)
    calls = json.load(open(os.path.join(d, "calls.json")))
    L = ftar.lib()
    for k, c in enumerate(calls):
        dt, es = DTYPES[c["dtype"]]
        x = np.fromfile(os.path.join(d, f"in_{rank}_{k}.bin"), dtype=np.uint8)
        nb, off = x.size, c["offset"]
        n = nb // es
        hs = np.full(nb + off + PAD, GUARD_S, dtype=np.uint8)
        hs[off:off + nb] = x
        hr = np.full(nb + off + PAD, GUARD_R, dtype=np.uint8)
        want_s = hs.copy()
        if c["host"]:
            fn = L.ftar_allreduce_rabenseifner_host if c["algo"] == "raben" else L.ftar_recursive_doubling_host
            rc = fn(hs.ctypes.data + off, hr.ctypes.data + off, n, dt, c["op"], comm._h)
            got_s, got_r = hs, hr
        else:
            fn = L.ftar_allreduce_rabenseifner if c["algo"] == "raben" else L.ftar_recursive_doubling
            ps = hip.upload(hs)
            pr = ps if c["inplace"] else hip.upload(hr)
            rc = fn(ps + off, pr + off, n, dt, c["op"], comm._h)
            got_r = hip.download(pr, hr)
            got_s = got_r if c["inplace"] else hip.download(ps, hs)
            hip.free(ps)
            if not c["inplace"]:
                hip.free(pr)
        guard_r = GUARD_S if c["inplace"] else GUARD_R
        intact = bool(np.all(got_r[:off] == guard_r) and np.all(got_r[off + nb:] == guard_r))
        if not c["inplace"]:
            intact = intact and bool(np.array_equal(got_s, want_s))
        st = comm.last_stats()
        got_r[off:off + nb].tofile(os.path.join(d, f"out_{rank}_{k}.bin"))
        with open(os.path.join(d, f"status_{rank}_{k}.txt"), "w") as f:
            f.write(f"{rc} {st.comm_size_after} {st.recoveries} {int(intact)}\n")
    comm.finalize()
    return 0


def main():
    d = os.environ["FTAR_PROBE_DIR"]
    ftar = load_package()
    hip = Hip(ftar.lib())
    if os.environ.get("PAIR_MODE", "sched") == "local":
        return run_local(ftar, hip, d)
    return run_sched(ftar, hip, d)


if __name__ == "__main__":
    sys.exit(main())
