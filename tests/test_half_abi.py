"""float16 / bfloat16 (FTAR_FLOAT16 = 16, FTAR_BFLOAT16 = 17) at the boundary, without a GPU.

* the product library admits the two types with SUM / PROD / MAX / MIN, answers MPI_ERR_OP to
  the logical and bitwise ops and MPI_ERR_ARG to every other type value;
* the host-sim test library, whose device layer reduces the four original types only, refuses
  them at the boundary instead of running them as something else;
* the Python binding maps the two torch dtypes;
* the work plans cover every element exactly once at 2-byte elements (tests/kernel_plan, a
  host program built with the address and undefined-behaviour sanitizers);
* half_model.py's restatement of the no-fault reduction trees -- which the GPU test reuses
  with 16-bit rounding -- is bit-equal to the oracle on float32.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import half_model as M
from plan_checks import run_planwalk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = 16, 17
RL_ARGS = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "fault-tolerant_amd"), "-j8"], check=True)
    return os.path.join(ROOT, "fault-tolerant_amd", "lib", "libftar.so")


def test_product_admits_the_half_types(built):
    L = ctypes.CDLL(built)
    L.ftar_reduce_local.argtypes = RL_ARGS
    for dt in (F16, BF16):
        for op in range(4):
            assert L.ftar_reduce_local(None, None, 0, dt, op, None) == 0, (dt, op)
        for op in range(4, 10):
            assert L.ftar_reduce_local(None, None, 0, dt, op, None) == 9, (dt, op)
        assert L.ftar_reduce_local(None, None, 0, dt, 10, None) == 13
    for dt in (4, 5, 15, 18):
        assert L.ftar_reduce_local(None, None, 0, dt, 0, None) == 13, dt


def test_header_and_binding_agree(ftar):
    import re
    src = open(os.path.join(ROOT, "include", "ftar.h")).read()
    assert int(re.search(r"FTAR_FLOAT16\s*=\s*(\d+)", src).group(1)) == ftar.FLOAT16 == F16
    assert int(re.search(r"FTAR_BFLOAT16\s*=\s*(\d+)", src).group(1)) == ftar.BFLOAT16 == BF16


def test_python_maps_the_torch_dtypes(ftar):
    import torch
    assert ftar._dtype_of(torch.zeros(1, dtype=torch.float16)) == ftar.FLOAT16
    assert ftar._dtype_of(torch.zeros(1, dtype=torch.bfloat16)) == ftar.BFLOAT16
    assert ftar._dtype_of(torch.zeros(1, dtype=torch.float32)) == ftar.FLOAT32
    with pytest.raises(ftar.FtarError):
        ftar._dtype_of(torch.zeros(1, dtype=torch.int16))


def test_hostsim_refuses_the_half_types(hostsim, monkeypatch):
    """The host-sim device layer has no 2-byte arithmetic: ftar_reduce_local and both Allreduce
    entry points of a one-rank comm return MPI_ERR_ARG, whatever the op, and touch nothing."""
    monkeypatch.setenv("FTAR_HOSTSIM_TAG", f"half{os.getpid()}")
    monkeypatch.delenv("FTAR_LAUNCHER", raising=False)
    L = ctypes.CDLL(os.path.join(hostsim, "libftar_hostsim.so"))
    L.ftar_reduce_local.argtypes = RL_ARGS
    L.ftar_init_rank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int]
    L.ftar_finalize.argtypes = [ctypes.c_void_p]
    entry = [L.ftar_allreduce_rabenseifner, L.ftar_recursive_doubling, L.ftar_allreduce_rabenseifner_host,
             L.ftar_recursive_doubling_host]
    for fn in entry:
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    for dt in (F16, BF16):
        for op in (0, 2, 4):
            assert L.ftar_reduce_local(None, None, 0, dt, op, None) == 13, (dt, op)
    assert L.ftar_reduce_local(None, None, 0, 1, 0, None) == 0  # float32 as before
    h = ctypes.c_void_p()
    assert L.ftar_init_rank(ctypes.byref(h), f"/ftar-half-{os.getpid()}".encode(), 0, 1, 0) == 0
    try:
        src = np.arange(64, dtype=np.float32)
        dst = np.full(64, -1.0, dtype=np.float32)
        for fn in entry:
            for dt in (F16, BF16):
                assert fn(src.ctypes.data, dst.ctypes.data, 8, dt, 0, h) == 13, (fn.__name__, dt)
        assert np.all(dst == -1.0)
    finally:
        L.ftar_finalize(h)


def test_plans_cover_two_byte_elements():
    """tests/kernel_plan at esize 2: plan_segments, plan_tree and plan_tree_batch, every misalignment
    of 0..7 elements, co-aligned and not; plain, and with checker and planners under ASan + UBSan.
    At least the 28468 cases of the walker this type came with."""
    assert run_planwalk(2) >= 28468


def _f32_pair(op):
    """MPI_Reduce_local's float32 combination, inout <op> in, as numpy (one IEEE operation;
    MAX / MIN: the oracle's (x > y) ? x : y with x = inout)."""
    return {0: lambda x, y: x + y, 1: lambda x, y: x * y, 2: lambda x, y: np.where(x > y, x, y),
            3: lambda x, y: np.where(x < y, x, y)}[op]


@pytest.mark.parametrize("p", [2, 4, 8])
@pytest.mark.parametrize("op", [0, 2])
def test_tree_model_is_the_oracles_tree(oracle, p, op):
    """The numpy restatement of the no-fault trees (Rabenseifner: recursive halving, each
    block in its owner's tree; recursive doubling: the last step with swapped roles) against
    the oracle, float32, count 1031: bit-equal for SUM on random values and for MAX on
    values with NaN / signed zeros / infinities, where the operand order shows."""
    import harness as H
    ins = oracle.random_inputs(p, 1031, seed=100 + p)
    if op == 2:
        ins = H.with_specials(ins, 7 + p)
    with np.errstate(all="ignore"):
        rb = M.raben_tree(ins, _f32_pair(op))
        rd = M.rd_tree(ins, _f32_pair(op))
    o = oracle.rabenseifner(ins, op=op)
    for w in range(p):
        assert np.array_equal(o.outputs[w].view(np.uint32), rb.view(np.uint32)), w
    o = oracle.recursive_doubling(ins, op=op)
    for w in range(p):
        assert np.array_equal(o.outputs[w].view(np.uint32), rd[w].view(np.uint32)), w
