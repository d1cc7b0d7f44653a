"""MAXLOC / MINLOC (16, 17) on MPI's pair types (FTAR_FLOAT_INT = 32, FTAR_2INT = 33,
FTAR_DOUBLE_INT = 34) at the boundary, without a GPU.

* the product library admits pair type x MAXLOC / MINLOC, answers MPI_ERR_OP to a pair type
  with any op 0..9 and to MAXLOC / MINLOC on any other type, MPI_ERR_ARG to everything unknown;
* header and Python binding agree on the values, and the header's structs have MPI's layouts
  (a C program compiled against the header);
* the host-sim test library, whose device layer reduces the four original types only, refuses
  the pair types at the boundary and touches nothing;
* the work plans cover every element exactly once at 8- and 16-byte elements
  (tests/kernel_plan: a host program, run plain and built with ASan + UBSan);
* pack_pairs / unpack_pairs round-trip on CPU tensors;
* the GPU test's two references agree with each other: the oracle's int64 MAX / MIN over the
  keys that encode (value, index) decodes to what the pairwise rule gives in half_model.py's
  trees.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from plan_checks import run_planwalk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_INT, TWO_INT, DOUBLE_INT = 32, 33, 34
PAIRS = (FLOAT_INT, TWO_INT, DOUBLE_INT)
MAXLOC, MINLOC = 16, 17
RL_ARGS = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "fault-tolerant_amd"), "-j8"], check=True)
    return os.path.join(ROOT, "fault-tolerant_amd", "lib", "libftar.so")


@pytest.fixture(scope="module")
def product(built):
    L = ctypes.CDLL(built)
    L.ftar_reduce_local.argtypes = RL_ARGS
    return L


def test_product_admits_the_pair_types(product):
    for dt in PAIRS:
        for op in (MAXLOC, MINLOC):
            assert product.ftar_reduce_local(None, None, 0, dt, op, None) == 0, (dt, op)


def test_product_answers_err_op_to_a_type_without_the_op(product):
    for dt in PAIRS:
        for op in range(10):
            assert product.ftar_reduce_local(None, None, 0, dt, op, None) == 9, (dt, op)
    for dt in (0, 1, 16):  # int32, float32, float16
        for op in (MAXLOC, MINLOC):
            assert product.ftar_reduce_local(None, None, 0, dt, op, None) == 9, (dt, op)


def test_product_answers_err_arg_to_the_unknown(product):
    for dt in PAIRS + (0, 1, 16):
        for op in (10, 11, 12, 13, 14, 15, 18):
            assert product.ftar_reduce_local(None, None, 0, dt, op, None) == 13, (dt, op)
    for dt in (18, 31, 35):
        for op in (0, MAXLOC, MINLOC):
            assert product.ftar_reduce_local(None, None, 0, dt, op, None) == 13, (dt, op)


def test_header_and_binding_agree(ftar):
    src = open(os.path.join(ROOT, "include", "ftar.h")).read()

    def value(name):
        return int(re.search(r"\b" + name + r"\s*=\s*(\d+)", src).group(1))

    assert value("FTAR_FLOAT_INT") == ftar.FLOAT_INT == FLOAT_INT
    assert value("FTAR_2INT") == ftar.TWO_INT == TWO_INT
    assert value("FTAR_DOUBLE_INT") == ftar.DOUBLE_INT == DOUBLE_INT
    assert value("FTAR_MAXLOC") == ftar.MAXLOC == MAXLOC
    assert value("FTAR_MINLOC") == ftar.MINLOC == MINLOC
    assert int(re.search(r"#define\s+FTAR_NOPS\s+(\d+)", src).group(1)) == 10
    assert "not offered" not in src


def test_header_structs_have_mpis_layouts(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "ftar.h"
#define ROW(T) printf(#T " %zu %zu %zu %zu\\n", sizeof(T), _Alignof(T), offsetof(T, v), offsetof(T, i))
int main(void) { ROW(ftar_float_int); ROW(ftar_2int); ROW(ftar_double_int); return 0; }
""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o",
                    str(exe)], check=True)
    rows = {r.split()[0]: tuple(map(int, r.split()[1:]))
            for r in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert rows == {"ftar_float_int": (8, 4, 0, 4), "ftar_2int": (8, 4, 0, 4), "ftar_double_int": (16, 8, 0, 8)}


def test_hostsim_refuses_the_pair_types(hostsim, monkeypatch):
    """The host-sim device layer has no pair kernels: ftar_reduce_local and all four Allreduce
    entry points of a one-rank comm return MPI_ERR_ARG and leave the output untouched."""
    monkeypatch.setenv("FTAR_HOSTSIM_TAG", f"pair{os.getpid()}")
    monkeypatch.delenv("FTAR_LAUNCHER", raising=False)
    L = ctypes.CDLL(os.path.join(hostsim, "libftar_hostsim.so"))
    L.ftar_reduce_local.argtypes = RL_ARGS
    L.ftar_init_rank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int]
    L.ftar_finalize.argtypes = [ctypes.c_void_p]
    entry = [L.ftar_allreduce_rabenseifner, L.ftar_recursive_doubling, L.ftar_allreduce_rabenseifner_host,
             L.ftar_recursive_doubling_host]
    for fn in entry:
        fn.argtypes = RL_ARGS
    for dt in PAIRS:
        for op in (MAXLOC, MINLOC, 0, 2):
            assert L.ftar_reduce_local(None, None, 0, dt, op, None) == 13, (dt, op)
    assert L.ftar_reduce_local(None, None, 0, 1, 0, None) == 0  # float32 as before
    assert L.ftar_reduce_local(None, None, 0, 1, MAXLOC, None) == 9
    h = ctypes.c_void_p()
    assert L.ftar_init_rank(ctypes.byref(h), f"/ftar-pair-{os.getpid()}".encode(), 0, 1, 0) == 0
    try:
        src = np.arange(64, dtype=np.int64)
        dst = np.full(64, -1, dtype=np.int64)
        for fn in entry:
            for dt in PAIRS:
                for op in (MAXLOC, MINLOC):
                    assert fn(src.ctypes.data, dst.ctypes.data, 8, dt, op, h) == 13, (fn.__name__, dt, op)
        assert np.all(dst == -1)
    finally:
        L.ftar_finalize(h)


def test_plans_cover_pair_elements():
    """tests/kernel_plan at esize 8 and 16: plan_segments, plan_tree and plan_tree_batch, windows at
    every misalignment the types' alignment allows, co-aligned and not: the plain build, and once
    more as a stand-alone program built, planners included, with ASan + UBSan.  At least the
    5280 + 1320 cases of the walker these types came with."""
    assert run_planwalk(8) >= 5280
    assert run_planwalk(16) >= 1320


@pytest.mark.parametrize("dt", PAIRS)
def test_pack_and_unpack_round_trip(ftar, dt):
    import torch
    vt = {FLOAT_INT: torch.float32, TWO_INT: torch.int32, DOUBLE_INT: torch.float64}[dt]
    g = torch.Generator().manual_seed(dt)
    for n in (0, 1, 5, 1031):
        if vt == torch.int32:
            v = torch.randint(-2**31, 2**31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
        else:
            v = (torch.randn(n, generator=g, dtype=torch.float64) * 1e3).to(vt)
            if n >= 5:
                v[:4] = torch.tensor([float("nan"), -0.0, float("inf"), float("-inf")], dtype=vt)
        i = torch.randint(-2**31, 2**31 - 1, (n,), generator=g, dtype=torch.int64)
        if n >= 5:
            i[:3] = torch.tensor([-2**31, 2**31 - 1, -1])
        t = ftar.pack_pairs(v, i, dt)
        assert t.is_contiguous() and tuple(t.shape) == (n, 2)
        assert t.dtype == (torch.int64 if dt == DOUBLE_INT else torch.int32)
        assert t.numel() * t.element_size() == n * (16 if dt == DOUBLE_INT else 8)
        # the bytes are the C struct's: value at 0, index at 4 (8), the padding zero
        raw = t.numpy().view(np.uint8).reshape(n, 16 if dt == DOUBLE_INT else 8)
        vs = v.element_size()
        assert np.array_equal(raw[:, :vs], v.numpy().view(np.uint8).reshape(n, vs))
        assert np.array_equal(raw[:, vs:vs + 4], i.to(torch.int32).numpy().view(np.uint8).reshape(n, 4))
        assert not raw[:, vs + 4:].any()
        v2, i2 = ftar.unpack_pairs(t, dt)
        assert v2.dtype == vt and i2.dtype == torch.int32
        assert np.array_equal(v2.numpy().view(np.uint8), v.numpy().view(np.uint8))  # bit for bit (NaN, -0)
        assert torch.equal(i2, i.to(torch.int32))
    with pytest.raises(ftar.FtarError):
        ftar.pack_pairs(torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32), FLOAT_INT)
    with pytest.raises(ftar.FtarError):
        ftar.pack_pairs(torch.zeros(3, dtype=vt), torch.zeros(3, dtype=torch.int32), 1)
    with pytest.raises(ftar.FtarError):
        ftar.unpack_pairs(torch.zeros((3, 3), dtype=torch.int32), dt)


@pytest.mark.parametrize("name", ["float_int", "double_int", "2int"])
def test_key_encoding_is_the_pairwise_rule(oracle, name):
    """test_gpu_pair.py checks the schedules against the oracle's int64 MAX / MIN of keys; here
    the decoded oracle result equals the header's rule applied in the no-fault trees, p = 4."""
    import half_model as M
    import test_gpu_pair as G
    for op, oop in ((G.MAXLOC, G.ORACLE_MAX), (G.MINLOC, G.ORACLE_MIN)):
        ins = G.keyed_inputs(name, 4, 1031, seed=op)
        o = oracle.rabenseifner(G.keys_of(ins, op), op=oop)
        G.assert_same_bytes(G.decode(o.outputs[0], op, name), M.raben_tree(ins, G.loc(op)), (name, op, "raben"))
        o = oracle.recursive_doubling(G.keys_of(ins, op), op=oop)
        for w in range(4):
            G.assert_same_bytes(G.decode(o.outputs[w], op, name), M.rd_tree(ins, G.loc(op))[w], (name, op, "rd", w))
