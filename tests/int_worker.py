"""TEST worker for the 8-, 16-bit and unsigned integer types (tests/test_gpu_int.py): every GPU
action of those tests happens in a process of this program, never in the pytest process.

Like pair_worker.py it binds the product library through the package and takes device memory from
the HIP runtime the library is linked with.  Buffers are raw bytes; windows are byte offsets,
counts are elements of the case's type (its ftar_dtype value and size travel in the case).

env: FTAR_PROBE_DIR (the job's directory), INT_MODE=

  local   run directly.  cases.json lists {"dtype", "es", "op", "n", "off_in", "off_io", "variant",
          "pinned"}; case i reads the whole buffers lin_i.bin and lio_i.bin (device memory, or
          pinned host memory), reduces n elements at the two byte offsets with
          ftar_set_reduce_variant(variant) and writes the whole in-out buffer to lout_i.bin.
          status.txt: one line "rc in_untouched" per case.

  sched   one rank under ftrun.  calls.json lists {"dtype", "es", "algo", "op", "inplace", "offset",
          "host"}: pair_worker.py's calls.  A call with "list": [[offset, count, inplace], ...]
          instead runs ftar_allreduce_multi over those windows of one guarded send buffer (count 0:
          a NULL entry), results into the same windows of a receive buffer (in place: of the send
          buffer); in_<rank>_<k>.bin is the dense concatenation, out_<rank>_<k>.bin the results in
          list order; its status line ends with ftar_stats.coalesced and the return codes of
          ftar_allreduce_multi_acc32 on the same list with the call's op and with MAXLOC.

  torch   one rank under ftrun: in_<rank>_0.bin as a torch.uint8 CUDA tensor through
          Comm.allreduce_rabenseifner (dtype from the tensor), BOR; then in_<rank>_1.bin as a
          torch.int16 tensor with dtype=INT16 named by the caller, MIN.
"""
import ctypes
import json
import os
import sys

import numpy as np

from half_worker import Hip, load_package

GUARD_S, GUARD_R, PAD = 0x5A, 0xEE, 32


def pinned(hip, a):
    """A copy of `a` in pinned host memory mapped at its own address: (pointer, numpy view)."""
    L = hip.L
    L.hipHostMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    p = ctypes.c_void_p()
    hip.ok(L.hipHostMalloc(ctypes.byref(p), max(a.nbytes, 16), 0), "hipHostMalloc")
    view = np.ctypeslib.as_array((ctypes.c_uint8 * a.nbytes).from_address(p.value))
    view[:] = a
    return p.value, view


def run_local(ftar, hip, d):
    hip.set_device(int(os.environ.get("FTAR_DEVICE", "0")))
    cases = json.load(open(os.path.join(d, "cases.json")))
    lines = []
    for i, c in enumerate(cases):
        a = np.fromfile(os.path.join(d, f"lin_{i}.bin"), dtype=np.uint8)
        b = np.fromfile(os.path.join(d, f"lio_{i}.bin"), dtype=np.uint8)
        assert c["off_in"] + c["n"] * c["es"] <= a.size and c["off_io"] + c["n"] * c["es"] <= b.size, c  # inside the buffers
        ftar.set_reduce_variant(c["variant"])
        if c.get("pinned"):
            pa, va = pinned(hip, a)
            pb, vb = pinned(hip, b)
        else:
            pa, pb = hip.upload(a), hip.upload(b)
        rc = ftar.lib().ftar_reduce_local(pa + c["off_in"], pb + c["off_io"], c["n"], c["dtype"], c["op"], None)
        if c.get("pinned"):
            hip.ok(hip.L.hipDeviceSynchronize(), "hipDeviceSynchronize")
            out, same = vb.copy(), bool(np.array_equal(va, a))
            hip.L.hipHostFree.argtypes = [ctypes.c_void_p]
            hip.L.hipHostFree(pa)
            hip.L.hipHostFree(pb)
        else:
            out = hip.download(pb, b)
            same = bool(np.array_equal(hip.download(pa, a), a))
            hip.free(pa)
            hip.free(pb)
        out.tofile(os.path.join(d, f"lout_{i}.bin"))
        lines.append(f"{rc} {int(same)}\n")
    with open(os.path.join(d, "status.txt"), "w") as f:
        f.writelines(lines)
    return 0


def run_list(ftar, hip, comm, c, x):
    """ftar_allreduce_multi over windows of one send buffer: (rc, outputs in list order, intact, tail)."""
    L, es = ftar.lib(), c["es"]
    end = max(off + n * es for off, n, _ in c["list"])
    hs = np.full(end + PAD, GUARD_S, dtype=np.uint8)
    at = 0
    for off, n, _ in c["list"]:
        hs[off:off + n * es] = x[at:at + n * es]
        at += n * es
    assert at == x.size
    hr = np.full(end + PAD, GUARD_R, dtype=np.uint8)
    ps, pr = hip.upload(hs), hip.upload(hr)
    k = len(c["list"])
    sb = (ctypes.c_void_p * k)(*[(ps + off) if n else None for off, n, _ in c["list"]])
    rb = (ctypes.c_void_p * k)(*[((ps if ip else pr) + off) if n else None for off, n, ip in c["list"]])
    cn = (ctypes.c_size_t * k)(*[n for _, n, _ in c["list"]])
    algo = 1 if c["algo"] == "raben" else 0
    acc = [L.ftar_allreduce_multi_acc32(algo, sb, rb, cn, k, c["dtype"], op, ctypes.c_float(1.0), comm._h) for op in (c["op"], 16)]
    rc = L.ftar_allreduce_multi(algo, sb, rb, cn, k, c["dtype"], c["op"], comm._h)
    coalesced = comm.last_stats().coalesced
    got_s, got_r = hip.download(ps, hs), hip.download(pr, hr)
    hip.free(ps)
    hip.free(pr)
    want_s, want_r = hs.copy(), hr.copy()
    outs = []
    for off, n, ip in c["list"]:
        src = got_s if ip else got_r
        outs.append(src[off:off + n * es].copy())
        (want_s if ip else want_r)[off:off + n * es] = outs[-1]
    intact = bool(np.array_equal(got_s, want_s) and np.array_equal(got_r, want_r))  # nothing outside the output windows
    return rc, np.concatenate(outs), intact, f"{coalesced} {acc[0]} {acc[1]}"


def run_sched(ftar, hip, d):
    rank = int(os.environ["FTAR_RANK"])
    comm = ftar.Comm.from_env()
    hip.set_device(comm.device)
    calls = json.load(open(os.path.join(d, "calls.json")))
    L = ftar.lib()
    for k, c in enumerate(calls):
        dt, es = c["dtype"], c["es"]
        x = np.fromfile(os.path.join(d, f"in_{rank}_{k}.bin"), dtype=np.uint8)
        tail = ""
        if "list" in c:
            rc, out, intact, tail = run_list(ftar, hip, comm, c, x)
        else:
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
            out = got_r[off:off + nb]
        st = comm.last_stats()
        out.tofile(os.path.join(d, f"out_{rank}_{k}.bin"))
        with open(os.path.join(d, f"status_{rank}_{k}.txt"), "w") as f:
            f.write(f"{rc} {st.comm_size_after} {st.recoveries} {int(intact)} {tail}\n")
    comm.finalize()
    return 0


def run_torch(ftar, d):
    import torch
    rank = int(os.environ["FTAR_RANK"])
    comm = ftar.Comm.from_env()
    torch.cuda.set_device(comm.device)
    x = torch.from_numpy(np.fromfile(os.path.join(d, f"in_{rank}_0.bin"), dtype=np.uint8)).cuda()
    out = torch.zeros_like(x)
    rc = comm.allreduce_rabenseifner(x, out, op=ftar.BOR)
    torch.cuda.synchronize()
    st = comm.last_stats()
    out.cpu().numpy().tofile(os.path.join(d, f"out_{rank}_0.bin"))
    with open(os.path.join(d, f"status_{rank}_0.txt"), "w") as f:
        f.write(f"{rc} {st.comm_size_after} {st.recoveries} 1\n")
    # a torch.int16 tensor: the binding does not map that dtype, the caller names the type
    y = torch.from_numpy(np.fromfile(os.path.join(d, f"in_{rank}_1.bin"), dtype=np.int16)).cuda()
    out = torch.zeros_like(y)
    rc = comm.allreduce_rabenseifner(y, out, dtype=ftar.INT16, op=ftar.MIN)
    torch.cuda.synchronize()
    st = comm.last_stats()
    out.cpu().numpy().tofile(os.path.join(d, f"out_{rank}_1.bin"))
    with open(os.path.join(d, f"status_{rank}_1.txt"), "w") as f:
        f.write(f"{rc} {st.comm_size_after} {st.recoveries} 1\n")
    comm.finalize()
    return 0


def main():
    d = os.environ["FTAR_PROBE_DIR"]
    ftar = load_package()
    mode = os.environ.get("INT_MODE", "sched")
    if mode == "torch":
        return run_torch(ftar, d)
    hip = Hip(ftar.lib())
    if mode == "local":
        return run_local(ftar, hip, d)
    return run_sched(ftar, hip, d)


if __name__ == "__main__":
    sys.exit(main())
