"""The 8-, 16-bit and unsigned integer types (FTAR_INT8 = 48 .. FTAR_UINT64 = 53) at the boundary,
without a GPU.

* the product library admits the six types with all ten ops 0..9, answers MPI_ERR_OP to MAXLOC /
  MINLOC on them and MPI_ERR_ARG to an unknown op; the values next to the block (47, 54) and the
  ones other tests pin (4, 5, 15, 18, 31, 35) stay MPI_ERR_ARG;
* header and Python binding agree on the values; the torch dtypes map;
* the host-sim test library, whose device layer reduces the four original types only, answers
  MPI_ERR_ARG at all six entry points and leaves the output untouched;
* ftar_allreduce_multi_acc32 keeps refusing them with the codes it documents.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import int_model as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_ARGS = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
AR_ARGS = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
MULTI_ARGS = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
ACC32_ARGS = MULTI_ARGS[:7] + [ctypes.c_float, ctypes.c_void_p]
SUCCESS, ERR_OP, ERR_ARG = 0, 9, 13


@pytest.fixture(scope="module")
def product():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "fault-tolerant_amd"), "-j8"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "fault-tolerant_amd", "lib", "libftar.so"))
    L.ftar_reduce_local.argtypes = RL_ARGS
    return L


def test_product_admits_the_six_types(product):
    for dt in I.TYPES:
        for op in range(10):
            assert product.ftar_reduce_local(None, None, 0, dt, op, None) == SUCCESS, (dt, op)
        for op in (16, 17):
            assert product.ftar_reduce_local(None, None, 0, dt, op, None) == ERR_OP, (dt, op)
        for op in (10, 15, 18, -1):
            assert product.ftar_reduce_local(None, None, 0, dt, op, None) == ERR_ARG, (dt, op)


def test_values_around_the_block_stay_unknown(product):
    for dt in (4, 5, 15, 18, 31, 35, 47, 54):
        for op in (0, 2, 16):
            assert product.ftar_reduce_local(None, None, 0, dt, op, None) == ERR_ARG, (dt, op)


def test_header_and_binding_agree(ftar):
    src = open(os.path.join(ROOT, "include", "ftar.h")).read()
    for name, want in (("INT8", 48), ("UINT8", 49), ("INT16", 50), ("UINT16", 51), ("UINT32", 52), ("UINT64", 53)):
        got = int(re.search(r"\bFTAR_" + name + r"\s*=\s*(\d+)", src).group(1))
        assert got == getattr(ftar, name) == getattr(I, name) == want, name


def test_python_maps_the_torch_dtypes(ftar):
    import torch
    assert ftar._dtype_of(torch.zeros(1, dtype=torch.int8)) == ftar.INT8
    assert ftar._dtype_of(torch.zeros(1, dtype=torch.uint8)) == ftar.UINT8
    for name, code in (("uint16", ftar.UINT16), ("uint32", ftar.UINT32), ("uint64", ftar.UINT64)):
        if hasattr(torch, name):  # newer torch only
            assert ftar._dtype_of(torch.zeros(1, dtype=getattr(torch, name))) == code
    assert ftar._dtype_of(torch.zeros(1, dtype=torch.int32)) == ftar.INT32  # as before
    with pytest.raises(ftar.FtarError):
        ftar._dtype_of(torch.zeros(1, dtype=torch.bool))
    with pytest.raises(ftar.FtarError):  # the storage view of raw 2-byte float bits: named by the caller (dtype=INT16)
        ftar._dtype_of(torch.zeros(1, dtype=torch.int16))


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def test_hostsim_refuses_the_six_types(hostsim, monkeypatch):
    """ftar_reduce_local, the four Allreduce entry points and ftar_allreduce_multi of a one-rank
    host-sim comm: MPI_ERR_ARG whatever the op (the type is unknown there, so also for MAXLOC),
    nothing written."""
    monkeypatch.setenv("FTAR_HOSTSIM_TAG", f"int{os.getpid()}")
    monkeypatch.delenv("FTAR_LAUNCHER", raising=False)
    L = ctypes.CDLL(os.path.join(hostsim, "libftar_hostsim.so"))
    L.ftar_reduce_local.argtypes = RL_ARGS
    L.ftar_init_rank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ftar_finalize.argtypes = [ctypes.c_void_p]
    L.ftar_allreduce_multi.argtypes = MULTI_ARGS
    entry = [L.ftar_allreduce_rabenseifner, L.ftar_recursive_doubling, L.ftar_allreduce_rabenseifner_host,
             L.ftar_recursive_doubling_host]
    for fn in entry:
        fn.argtypes = AR_ARGS
    h = ctypes.c_void_p()
    assert L.ftar_init_rank(ctypes.byref(h), f"/ftar-int-{os.getpid()}".encode(), 0, 1, 0) == 0
    try:
        src = np.arange(64, dtype=np.int64)
        dst = np.full(64, -1, dtype=np.int64)
        io = dst.copy()
        counts = (ctypes.c_size_t * 2)(8, 8)
        for dt in I.TYPES:
            for op in (0, 2, 4, 9, 16):
                assert L.ftar_reduce_local(src.ctypes.data, io.ctypes.data, 8, dt, op, None) == ERR_ARG, (dt, op)
                for fn in entry:
                    assert fn(src.ctypes.data, dst.ctypes.data, 8, dt, op, h) == ERR_ARG, (fn.__name__, dt, op)
                for algo in (0, 1):
                    rc = L.ftar_allreduce_multi(algo, _ptrs([src[:8], src[8:16]]), _ptrs([dst[:8], dst[8:16]]), counts, 2, dt, op, h)
                    assert rc == ERR_ARG, (algo, dt, op)
        assert np.all(dst == -1) and np.all(io == -1)
        assert L.ftar_reduce_local(None, None, 0, 0, 0, None) == SUCCESS  # int32 as before
    finally:
        L.ftar_finalize(h)


def test_acc32_refuses_the_six_types(product):
    """Without a GPU there is no comm, and a NULL comm is MPI_ERR_ARG before anything else, which is
    also the code for a dtype that is not a 2-byte float; nothing is touched.  The documented order
    with a comm -- the op / dtype check first (MAXLOC on an integer type: MPI_ERR_OP), then the
    dtype -- is checked on the GPU (test_gpu_int.py, the list job)."""
    product.ftar_allreduce_multi_acc32.argtypes = ACC32_ARGS
    a = np.zeros(8, dtype=np.int64)
    counts = (ctypes.c_size_t * 1)(4)
    for dt in I.TYPES:
        for op in (0, 2, 7, 16, 10):
            rc = product.ftar_allreduce_multi_acc32(1, _ptrs([a]), _ptrs([a]), counts, 1, dt, op, 1.0, None)
            assert rc == ERR_ARG, (dt, op, rc)
    assert np.all(a == 0)
