"""Local reduce at 2 x 256 MiB operands, bench.py's method, for any element type (README.md here).

    python profiles/pair_types/measure.py <libftar.so> <label> <dtype:op:variant>[,...]

dtype: f32 | float_int | 2int | double_int; op: the ftar_op number; variant: 0 register-streaming,
1 LDS kernel.  Four rotating pairs of 256 MiB operands (2 GiB: beyond the 256 MiB Infinity
Cache), 8 warm-up launches, then 5 regions of 40 launches, each between one event pair on the
null stream the kernel runs on; GB/s = 3 x 256 MiB / time per launch.  One JSON line per case:
median, min and max of the 5 regions, and a check of the first pair's first elements.
"""
import ctypes
import json
import sys

import numpy as np

BYTES, PAIRS, WARM, REGIONS, PER = 256 << 20, 4, 8, 5, 40
H2D, D2H = 1, 2
TYPES = {"f32": (1, np.dtype("<f4")),
         "float_int": (32, np.dtype([("v", "<f4"), ("i", "<i4")])),
         "2int": (33, np.dtype([("v", "<i4"), ("i", "<i4")])),
         "double_int": (34, np.dtype([("v", "<f8"), ("i", "<i4"), ("pad", "<u4")]))}


def main():
    path, label, cases = sys.argv[1], sys.argv[2], sys.argv[3].split(",")
    L = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    L.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    L.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    L.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    L.hipEventRecord.argtypes = [vp, vp]
    L.hipEventSynchronize.argtypes = [vp]
    L.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    L.ftar_reduce_local.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, vp]

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"{what}: error {rc}")

    ok(L.hipSetDevice(0), "hipSetDevice")
    bufs = []
    for _ in range(2 * PAIRS):
        p = vp()
        ok(L.hipMalloc(ctypes.byref(p), BYTES), "hipMalloc")
        bufs.append(p.value)
    e0, e1 = vp(), vp()
    ok(L.hipEventCreate(ctypes.byref(e0)), "hipEventCreate")
    ok(L.hipEventCreate(ctypes.byref(e1)), "hipEventCreate")
    rng = np.random.default_rng(1)
    for case in cases:
        name, op, variant = case.split(":")
        dt, nd = TYPES[name]
        op, variant, n = int(op), int(variant), BYTES // nd.itemsize
        host = []
        for _ in range(2):  # the in and the in-out operand, the same for every pair
            a = np.zeros(n, dtype=nd)
            if nd.names:
                a["v"] = rng.integers(-1000, 1000, size=n)
                a["i"] = rng.integers(0, 64, size=n)
            else:
                a[:] = rng.integers(-4, 5, size=n)
            host.append(a)
        for k, b in enumerate(bufs):
            ok(L.hipMemcpy(b, host[k & 1].ctypes.data, BYTES, H2D), "hipMemcpy")
        ok(L.ftar_set_reduce_variant(variant), "ftar_set_reduce_variant")

        def launch(j):
            ok(L.ftar_reduce_local(bufs[2 * (j % PAIRS)], bufs[2 * (j % PAIRS) + 1], n, dt, op, None), "ftar_reduce_local")

        for j in range(WARM):
            launch(j)
        ok(L.hipDeviceSynchronize(), "hipDeviceSynchronize")
        rates = []
        for _ in range(REGIONS):
            ok(L.hipEventRecord(e0, None), "hipEventRecord")
            for j in range(PER):
                launch(j)
            ok(L.hipEventRecord(e1, None), "hipEventRecord")
            ok(L.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = ctypes.c_float()
            ok(L.hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
            rates.append(3 * BYTES / (ms.value / PER * 1e-3) / 1e9)
        got = np.zeros(4096, dtype=nd)
        ok(L.hipMemcpy(got.ctypes.data, bufs[1], got.nbytes, D2H), "hipMemcpy")
        x, y = host[1][:4096], host[0][:4096]  # in-out, in
        if nd.names:  # the select is idempotent: after any number of launches, the first one's result
            t = ((x["v"] > y["v"]) if op == 16 else (x["v"] < y["v"])) | ((x["v"] == y["v"]) & (x["i"] < y["i"]))
            want = y.copy()
            want[t] = x[t]
            good = bool(np.array_equal(got.view(np.uint8), want.view(np.uint8)))
        else:
            good = bool(np.all(np.isfinite(got)))
        rates.sort()
        print(json.dumps({"lib": label, "variant": variant, "dtype": name, "op": op,
                          "GBps_median": round(rates[REGIONS // 2], 1), "GBps_min": round(rates[0], 1),
                          "GBps_max": round(rates[-1], 1), "checked": good}), flush=True)


if __name__ == "__main__":
    main()
