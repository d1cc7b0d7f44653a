"""TEST worker for the 2-byte float types (tests/test_gpu_half.py): every GPU action of those
tests happens in a process of this program, never in the pytest process.

It binds the product library through the package (as bench.py does) and moves raw uint16
files; device memory comes from the HIP runtime the library itself is linked with (no torch:
a rank starts in a fraction of a second).

env: FTAR_PROBE_DIR (the job's directory), HALF_DTYPE=f16|bf16, HALF_MODE=

  local   run directly.  cases.json lists {"dtype", "op", "n", "off_in", "off_io", "variant"}
          (dtype: the case's own, default HALF_DTYPE); case i reads the whole buffers lin_i.bin
          and lio_i.bin, reduces n elements at the two element offsets with
          ftar_set_reduce_variant(variant) and writes the whole in-out buffer to lout_i.bin.
          status.txt: one line "rc in_untouched" per case.

  sched   one rank under ftrun.  calls.json lists {"algo": "raben"|"rd", "op", "inplace",
          "offset", "host"}; call k reads in_<rank>_<k>.bin, puts it at element `offset` of a
          guarded buffer (device memory, or pageable host memory for the *_host entry points),
          runs the Allreduce and writes out_<rank>_<k>.bin and status_<rank>_<k>.txt:
          "rc comm_size_after recoveries intact" (intact: the guards around both windows, and
          the send window unless in place, still hold what was put there).
"""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"f16": 16, "bf16": 17}
GUARD_S, GUARD_R, PAD = 0x5A5A, 0xEEEE, 16
H2D, D2H = 1, 2


class Hip:
    """The few runtime calls needed, found through the library's own dependencies."""

    def __init__(self, lib):
        vp = ctypes.c_void_p
        self.L = lib
        lib.hipSetDevice.argtypes = [ctypes.c_int]
        lib.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
        lib.hipFree.argtypes = [vp]
        lib.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
        lib.hipDeviceSynchronize.argtypes = []

    def ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with HIP error {rc}")

    def set_device(self, d):
        self.ok(self.L.hipSetDevice(d), "hipSetDevice")

    def upload(self, a):
        p = ctypes.c_void_p()
        self.ok(self.L.hipMalloc(ctypes.byref(p), max(a.nbytes, 16)), "hipMalloc")
        if a.nbytes:
            self.ok(self.L.hipMemcpy(p, a.ctypes.data, a.nbytes, H2D), "hipMemcpy")
        return p.value

    def download(self, p, like):
        out = np.empty_like(like)
        self.ok(self.L.hipDeviceSynchronize(), "hipDeviceSynchronize")
        if out.nbytes:
            self.ok(self.L.hipMemcpy(out.ctypes.data, p, out.nbytes, D2H), "hipMemcpy")
        return out

    def free(self, p):
        self.L.hipFree(p)


def load_package():
    spec = importlib.util.spec_from_file_location("ftar_amd", os.path.join(ROOT, "fault-tolerant_amd", "__init__.py"))
    ftar = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ftar)
    return ftar


def run_local(ftar, hip, d, default_dt):
    hip.set_device(int(os.environ.get("FTAR_DEVICE", "0")))
    cases = json.load(open(os.path.join(d, "cases.json")))
    lines = []
    for i, c in enumerate(cases):
        dt = DTYPES[c.get("dtype", default_dt)]
        a = np.fromfile(os.path.join(d, f"lin_{i}.bin"), dtype=np.uint16)
        b = np.fromfile(os.path.join(d, f"lio_{i}.bin"), dtype=np.uint16)
        assert c["off_in"] + c["n"] <= a.size and c["off_io"] + c["n"] <= b.size, c  # stay inside the buffers
        ftar.set_reduce_variant(c["variant"])
        pa, pb = hip.upload(a), hip.upload(b)
        rc = ftar.lib().ftar_reduce_local(pa + 2 * c["off_in"], pb + 2 * c["off_io"], c["n"], dt, c["op"], None)
        out = hip.download(pb, b)
        same = bool(np.array_equal(hip.download(pa, a), a))
        out.tofile(os.path.join(d, f"lout_{i}.bin"))
        hip.free(pa)
        hip.free(pb)
        lines.append(f"{rc} {int(same)}\n")
    with open(os.path.join(d, "status.txt"), "w") as f:
        f.writelines(lines)
    return 0


def run_sched(ftar, hip, d, dt):
    rank = int(os.environ["FTAR_RANK"])
    comm = ftar.Comm.from_env()
    hip.set_device(comm.device)
    calls = json.load(open(os.path.join(d, "calls.json")))
    L = ftar.lib()
    for k, c in enumerate(calls):
        x = np.fromfile(os.path.join(d, f"in_{rank}_{k}.bin"), dtype=np.uint16)
        n, off = x.size, c["offset"]
        hs = np.full(n + off + PAD, GUARD_S, dtype=np.uint16)
        hs[off:off + n] = x
        hr = np.full(n + off + PAD, GUARD_R, dtype=np.uint16)
        want_s = hs.copy()
        if c["host"]:
            fn = L.ftar_allreduce_rabenseifner_host if c["algo"] == "raben" else L.ftar_recursive_doubling_host
            rc = fn(hs.ctypes.data + 2 * off, hr.ctypes.data + 2 * off, n, dt, c["op"], comm._h)
            got_s, got_r = hs, hr
        else:
            fn = L.ftar_allreduce_rabenseifner if c["algo"] == "raben" else L.ftar_recursive_doubling
            ps = hip.upload(hs)
            pr = ps if c["inplace"] else hip.upload(hr)
            rc = fn(ps + 2 * off, pr + 2 * off, n, dt, c["op"], comm._h)
            got_r = hip.download(pr, hr)
            got_s = got_r if c["inplace"] else hip.download(ps, hs)
            hip.free(ps)
            if not c["inplace"]:
                hip.free(pr)
        guard_r = GUARD_S if c["inplace"] else GUARD_R
        intact = bool(np.all(got_r[:off] == guard_r) and np.all(got_r[off + n:] == guard_r))
        if not c["inplace"]:
            intact = intact and bool(np.array_equal(got_s, want_s))
        st = comm.last_stats()
        got_r[off:off + n].tofile(os.path.join(d, f"out_{rank}_{k}.bin"))
        with open(os.path.join(d, f"status_{rank}_{k}.txt"), "w") as f:
            f.write(f"{rc} {st.comm_size_after} {st.recoveries} {int(intact)}\n")
    comm.finalize()
    return 0


def main():
    d = os.environ["FTAR_PROBE_DIR"]
    name = os.environ.get("HALF_DTYPE", "bf16")
    ftar = load_package()
    hip = Hip(ftar.lib())
    if os.environ.get("HALF_MODE", "sched") == "local":
        return run_local(ftar, hip, d, name)
    return run_sched(ftar, hip, d, DTYPES[name])


if __name__ == "__main__":
    sys.exit(main())
