"""ftar_allreduce_multi at the boundary, without a GPU.

* the symbol is exported by the product library and listed in csrc/ftar.map; header, Python
  binding and Stats agree (FTAR_ALGO_*, FTAR_MULTI_MAX, the `coalesced` field at the end);
* on a one-rank host-sim comm every refusal returns its code and leaves sentinel-filled outputs
  untouched; a valid call returns every rbufs[i] equal to sbufs[i] with the guard bytes on both
  sides of every buffer intact;
* the gather kernel's tile -> entry mapping covers every packed byte exactly once
  (tests/kernel_plan_multi: a host program, run plain and built with ASan + UBSan);
* the binding refuses mixed dtypes and non-contiguous tensors before anything is called.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
MULTI_ARGS = [ctypes.c_int, ctypes.POINTER(VP), ctypes.POINTER(VP), ctypes.POINTER(SZ), ctypes.c_int, ctypes.c_int,
              ctypes.c_int, VP]
RD, RABEN = 0, 1


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "fault-tolerant_amd"), "-j8"], check=True)
    return os.path.join(ROOT, "fault-tolerant_amd", "lib", "libftar.so")


def test_symbol_is_exported_and_mapped(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "ftar_allreduce_multi" and " T " in line for line in out.splitlines())
    assert re.search(r"\bftar_allreduce_multi;", open(os.path.join(ROOT, "fault-tolerant_amd", "csrc", "ftar.map")).read())
    # the mover is the device layer's kernel launch in the product (the fallback is host-sim's)
    syms = subprocess.run(["nm", built], capture_output=True, text=True, check=True).stdout
    assert re.search(r" [Tt] fdev_gather$", syms, flags=re.M)
    assert "gather_kernel" in syms


def test_header_binding_and_stats_agree(ftar):
    src = open(os.path.join(ROOT, "include", "ftar.h")).read()
    assert int(re.search(r"\bFTAR_ALGO_RD\s*=\s*(\d+)", src).group(1)) == ftar.ALGO_RD == RD
    assert int(re.search(r"\bFTAR_ALGO_RABENSEIFNER\s*=\s*(\d+)", src).group(1)) == ftar.ALGO_RABENSEIFNER == RABEN
    assert int(re.search(r"#define\s+FTAR_MULTI_MAX\s+(\d+)", src).group(1)) == ftar.MULTI_MAX == 1024
    body = re.search(r"typedef struct\s*\{([^{}]*)\}\s*ftar_stats\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S)).group(1)
    assert re.findall(r"(\w+)\s*;", body)[-1] == "coalesced" == ftar.Stats._fields_[-1][0]
    assert hasattr(ftar.Comm, "allreduce_multi")


@pytest.fixture()
def solo(hostsim, monkeypatch):
    """The host-sim library and a one-rank comm of it."""
    monkeypatch.setenv("FTAR_HOSTSIM_TAG", f"multi{os.getpid()}")
    monkeypatch.delenv("FTAR_LAUNCHER", raising=False)
    monkeypatch.delenv("FTAR_KILL", raising=False)
    L = ctypes.CDLL(os.path.join(hostsim, "libftar_hostsim.so"))
    L.ftar_allreduce_multi.argtypes = MULTI_ARGS
    L.ftar_init_rank.argtypes = [ctypes.POINTER(VP), ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ftar_finalize.argtypes = [VP]
    L.ftar_allreduce_rabenseifner.argtypes = L.ftar_recursive_doubling.argtypes = [VP, VP, SZ, ctypes.c_int, ctypes.c_int, VP]
    h = VP()
    assert L.ftar_init_rank(ctypes.byref(h), f"/ftar-multi-{os.getpid()}".encode(), 0, 1, 0) == 0
    yield L, h
    L.ftar_finalize(h)


GUARD = 8


def _bufs(counts, dtype=np.float32):
    """Per entry an input and a sentinel-filled output, each with GUARD elements on both sides."""
    rng = np.random.default_rng(5)
    ins, outs = [], []
    for c in counts:
        a = np.full(c + 2 * GUARD, 77, dtype=dtype)
        a[GUARD:GUARD + c] = rng.integers(-100, 100, size=c).astype(dtype)
        ins.append(a)
        outs.append(np.full(c + 2 * GUARD, -5, dtype=dtype))
    return ins, outs


def _args(ins, outs, counts):
    n = len(counts)
    es = ins[0].itemsize if ins else 4
    sb = (VP * max(n, 1))(*[a.ctypes.data + GUARD * es for a in ins])
    rb = (VP * max(n, 1))(*[a.ctypes.data + GUARD * es for a in outs])
    return sb, rb, (SZ * max(n, 1))(*counts)


def test_refusals_touch_nothing(solo):
    L, h = solo
    counts = [3, 5, 0, 2]
    ins, outs = _bufs(counts)
    sb, rb, ct = _args(ins, outs, counts)
    big = 1025
    bsb, brb, bct = (VP * big)(*[ins[0].ctypes.data] * big), (VP * big)(*[outs[0].ctypes.data] * big), (SZ * big)(*[0] * big)
    for algo in (RD, RABEN):
        assert L.ftar_allreduce_multi(algo, sb, rb, ct, 0, 1, 0, h) == 13           # nbufs 0
        assert L.ftar_allreduce_multi(algo, sb, rb, ct, -1, 1, 0, h) == 13
        assert L.ftar_allreduce_multi(algo, bsb, brb, bct, big, 1, 0, h) == 13      # nbufs 1025
        assert L.ftar_allreduce_multi(algo, None, rb, ct, 4, 1, 0, h) == 13         # NULL arrays
        assert L.ftar_allreduce_multi(algo, sb, None, ct, 4, 1, 0, h) == 13
        assert L.ftar_allreduce_multi(algo, sb, rb, None, 4, 1, 0, h) == 13
        assert L.ftar_allreduce_multi(algo, sb, rb, ct, 4, 1, 0, None) == 13        # no comm
        assert L.ftar_allreduce_multi(algo, sb, rb, ct, 4, 1, 4, h) == 9            # LAND on float32
        assert L.ftar_allreduce_multi(algo, sb, rb, ct, 4, 5, 0, h) == 13           # dtype 5
        assert L.ftar_allreduce_multi(algo, None, None, None, 0, 1, 4, h) == 9      # the op check comes first
        # a non-empty entry with a NULL pointer (the device entry points' memory rule)
        nsb = (VP * 4)(*[sb[0], None, sb[2], sb[3]])
        assert L.ftar_allreduce_multi(algo, nsb, rb, ct, 4, 1, 0, h) == 13
        # overlapping outputs: entry 1's output starts inside entry 0's
        orb = (VP * 4)(*[rb[0], rb[0] + 4, rb[2], rb[3]])
        assert L.ftar_allreduce_multi(algo, sb, orb, ct, 4, 1, 0, h) == 13
        orb = (VP * 4)(*[rb[1] + 4 * 4, rb[1], rb[2], rb[3]])  # ... and the other way round, by one element
        assert L.ftar_allreduce_multi(algo, sb, orb, ct, 4, 1, 0, h) == 13
    for bad in (2, -1, 7):
        assert L.ftar_allreduce_multi(bad, sb, rb, ct, 4, 1, 0, h) == 13            # unknown algo
    # a total of 0 elements: what the plain call with count == 0 returns (Raben: MPI_ERR_UNKNOWN)
    zc = (SZ * 4)(0, 0, 0, 0)
    assert L.ftar_allreduce_multi(RABEN, sb, rb, zc, 4, 1, 0, h) == 14
    assert L.ftar_allreduce_rabenseifner(None, None, 0, 1, 0, h) == 14
    assert L.ftar_allreduce_multi(RD, sb, rb, zc, 4, 1, 0, h) == L.ftar_recursive_doubling(None, None, 0, 1, 0, h)
    for o in outs:
        assert np.all(o == -5)
    for a in ins:
        assert np.all(a[:GUARD] == 77) and np.all(a[-GUARD:] == 77)


@pytest.mark.parametrize("algo", [RD, RABEN])
@pytest.mark.parametrize("dtype,code", [(np.float32, 1), (np.int64, 2)])
def test_valid_call_on_one_rank_is_a_copy(solo, ftar, algo, dtype, code):
    L, h = solo
    L.ftar_last_stats.argtypes = [VP, ctypes.POINTER(ftar.Stats)]
    counts = [1, 3, 0, 5, 4093, 4099, 2, 2, 2] + [1 + (i * 5) % 7 for i in range(40)]
    ins, outs = _bufs(counts, dtype)
    keep = [a.copy() for a in ins]
    sb, rb, ct = _args(ins, outs, counts)
    sb[2], rb[2] = 8, 8  # the empty entry's pointers are not looked at
    assert L.ftar_allreduce_multi(algo, sb, rb, ct, len(counts), code, 0, h) == 0
    st = ftar.Stats()
    assert L.ftar_last_stats(h, ctypes.byref(st)) == 0
    assert st.coalesced == sum(1 for c in counts if c) and st.comm_size_after == 1
    for c, a, k, o in zip(counts, ins, keep, outs):
        assert np.array_equal(a, k)                                            # inputs and their guards
        assert np.array_equal(o[GUARD:GUARD + c], a[GUARD:GUARD + c])
        assert np.all(o[:GUARD] == -5) and np.all(o[GUARD + c:] == -5)         # guards on both sides
    # in place, and exactly one non-empty entry (straight through: nothing gathered)
    one = (SZ * len(counts))(*[0] * len(counts))
    one[4] = counts[4]
    assert L.ftar_allreduce_multi(algo, sb, sb, one, len(counts), code, 0, h) == 0
    assert L.ftar_last_stats(h, ctypes.byref(st)) == 0 and st.coalesced == 0
    assert L.ftar_allreduce_multi(algo, sb, sb, ct, len(counts), code, 0, h) == 0
    assert L.ftar_last_stats(h, ctypes.byref(st)) == 0 and st.coalesced == sum(1 for c in counts if c)
    for a, k in zip(ins, keep):
        assert np.array_equal(a, k)


def test_tile_mapping_covers_every_packed_byte():
    """tests/kernel_plan_multi: the plain build, and once more as a stand-alone program whose host
    code is built with ASan + UBSan (nothing is preloaded)."""
    d = os.path.join(ROOT, "tests", "kernel_plan_multi")
    subprocess.run(["make", "-s", "-C", d], check=True)
    san = os.path.join(d, "_build", "planmulti_check_san")
    flags = subprocess.run(["nm", san], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in flags and "__ubsan_handle" in flags  # really built with the sanitizers
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    for exe in (os.path.join(d, "_build", "planmulti_check"), san):
        cp = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert cp.returncode == 0, cp.stdout + cp.stderr[-3000:]
        assert cp.stdout.startswith("OK ") and int(cp.stdout.split()[1]) > 100000


def test_binding_refuses_mixed_and_strided_tensors(hostsim, monkeypatch):
    """With the host-sim library bound (a private copy of the package: its "device" memory is host
    memory, so plain CPU tensors are buffers the binding accepts) every refusal is the one named,
    raised before anything is called; a valid list then goes through."""
    import importlib.util
    import torch
    monkeypatch.setenv("FTAR_HOSTSIM_TAG", f"multib{os.getpid()}")
    monkeypatch.delenv("FTAR_LAUNCHER", raising=False)
    monkeypatch.delenv("FTAR_KILL", raising=False)
    spec = importlib.util.spec_from_file_location("ftar_amd_multi_binding", os.path.join(ROOT, "fault-tolerant_amd", "__init__.py"))
    ftar = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ftar)
    ftar.use_test_library(os.path.join(hostsim, "libftar_hostsim.so"))

    class NoCall(ftar.Comm):
        def __init__(self):
            self._h = None

    c = NoCall()
    a, b = torch.zeros(4, dtype=torch.float32), torch.zeros(4, dtype=torch.int32)
    assert ftar._ptr(a) == a.data_ptr()  # a contiguous CPU tensor is accepted here
    with pytest.raises(ftar.FtarError, match="one dtype"):
        c.allreduce_multi([a, b])
    with pytest.raises(ftar.FtarError, match="contiguous"):
        c.allreduce_multi([a, torch.zeros(8, dtype=torch.float32)[::2]])
    with pytest.raises(ftar.FtarError, match="contiguous"):
        c.allreduce_multi([a], out=[torch.zeros(8, dtype=torch.float32)[::2]])
    with pytest.raises(ftar.FtarError, match="as many outputs"):
        c.allreduce_multi([a], out=[a, a])
    with pytest.raises(ftar.FtarError, match="size differs"):
        c.allreduce_multi([a], out=[torch.zeros(5, dtype=torch.float32)])
    with pytest.raises(ftar.FtarError, match="unknown algo"):
        c.allreduce_multi([a], algo="ring")
    with pytest.raises(ftar.FtarError, match="tensors"):
        c.allreduce_multi([])
    with pytest.raises(ftar.FtarError, match="unsupported dtype"):
        c.allreduce_multi([torch.zeros(4, dtype=torch.int16)])  # _dtype_of keeps its mapping
    # pair types: only the layout pack_pairs produces -- (n, 2) int32, for DOUBLE_INT (n, 2) int64
    pairs = ftar.pack_pairs(torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32), ftar.DOUBLE_INT)
    for bad in (torch.zeros((3, 2), dtype=torch.float32), torch.zeros((3, 2), dtype=torch.int32), torch.zeros(6, dtype=torch.int64),
                torch.zeros((3, 4), dtype=torch.int64)[:, :2]):
        with pytest.raises(ftar.FtarError, match="pack_pairs"):
            c.allreduce_multi([bad], op=ftar.MAXLOC, dtype=ftar.DOUBLE_INT)
    with pytest.raises(ftar.FtarError, match="pack_pairs"):
        c.allreduce_multi([pairs], op=ftar.MAXLOC, dtype=ftar.FLOAT_INT)
    with pytest.raises(ftar.FtarError, match="not a pair type"):
        c.allreduce_multi([a], dtype=ftar.FLOAT32)
    # a valid list on a one-rank comm: the result is the input
    comm = ftar.Comm.init_rank(f"/ftar-multi-bind-{os.getpid()}", 0, 1, 0)
    try:
        xs = [torch.arange(5, dtype=torch.float32), torch.zeros(0), torch.arange(3, dtype=torch.float32) + 7]
        outs = [torch.full_like(x, -1) for x in xs]
        assert comm.allreduce_multi(xs, out=outs, algo="rd") == 0
        assert all(torch.equal(o, x) for o, x in zip(outs, xs)) and comm.last_stats().coalesced == 2
    finally:
        comm.finalize()
