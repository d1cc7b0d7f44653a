"""ftar_allreduce_multi_acc32 without a GPU.

* the numpy model the GPU tests compare against (tests/acc32_runner.py: widen / narrow) agrees with
  torch's CPU conversions: on all 65536 patterns of both types, on 2^20 random float32 bit
  patterns, and on every float32 that lies exactly halfway between two neighbouring 16-bit values
  (bfloat16: all of them; float16: every mantissa at a sample of exponents, the subnormal range
  and the overflow threshold included);
* the converting kernel's tile -> entry -> piece walk (tests/kernel_plan_acc32: a host program, run
  plain and built with ASan + UBSan as a stand-alone binary; nothing is preloaded);
* the symbol is exported by the product library and the host-sim library and listed in
  csrc/ftar.map; the device hook is the product's kernel launch; header and binding agree;
* on the host-sim library, which has no 2-byte float types, both types return FTAR_ERR_ARG with
  nothing touched, and the argument-error order holds where it is reachable there;
* the binding refuses what it must before anything is called.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import acc32_runner as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
ACC32_ARGS = [ctypes.c_int, ctypes.POINTER(VP), ctypes.POINTER(VP), ctypes.POINTER(SZ), ctypes.c_int, ctypes.c_int,
              ctypes.c_int, ctypes.c_float, VP]
RD, RABEN = 0, 1
ERR_OP, ERR_ARG = 9, 13


@pytest.fixture(autouse=True, scope="module")
def declared():
    """Everything here describes one entry point; without its declaration there is nothing to describe."""
    assert "ftar_allreduce_multi_acc32" in open(os.path.join(ROOT, "include", "ftar.h")).read()


def _torch_dt(dt):
    import torch
    return torch.float16 if dt == A.F16 else torch.bfloat16


def _torch_narrow(f32, dt):
    import torch
    return torch.from_numpy(f32.copy()).to(_torch_dt(dt)).view(torch.int16).numpy().view(np.uint16)


def _torch_widen(u16, dt):
    import torch
    return torch.from_numpy(u16.view(np.int16).copy()).view(_torch_dt(dt)).to(torch.float32).numpy()


@pytest.mark.parametrize("name", list(A.TYPES))
def test_model_on_every_16_bit_pattern(name):
    dt = A.TYPES[name]
    u = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    w, t = A.widen(u, dt), _torch_widen(u, dt)
    nan = np.isnan(t)
    assert np.array_equal(np.isnan(w), nan) and 0 < nan.sum() < 4096
    assert np.array_equal(w[~nan].view(np.uint32), t[~nan].view(np.uint32))  # widening: bit-exact
    back = A.narrow(w, dt)
    assert np.array_equal(back[~nan], u[~nan])                               # narrow(widen(x)) == x
    assert np.all(np.isnan(A.widen(back[nan], dt)))                          # a NaN stays a NaN


def _halfway(dt):
    """Every float32 exactly halfway between two neighbouring values of the 16-bit type (at the
    sampled exponents), both signs."""
    if dt == A.BF16:  # the float32 whose low half is exactly 0x8000, for every finite upper half
        hi = np.arange(65536, dtype=np.uint32)
        u = (hi << 16) | 0x8000
        return u[((hi >> 7) & 0xFF) != 0xFF].view(np.float32)
    m = np.arange(1024, dtype=np.uint32)
    parts = []
    # normal float16 exponents -14 .. 15 (float32 biased 113 .. 142): a sample, both ends included;
    # at 142 the last one is 65520, halfway between 65504 and the overflow to inf
    for e32 in (113, 114, 120, 127, 128, 135, 141, 142):
        parts.append(((e32 << 23) | (m << 13) | 0x1000).astype(np.uint32).view(np.float32))
    # the subnormal range: (k + 1/2) * 2^-24, k = 0 .. 1023 (exact in float32)
    parts.append(((m.astype(np.float64) + 0.5) * 2.0 ** -24).astype(np.float32))
    x = np.concatenate(parts)
    return np.concatenate([x, -x])


@pytest.mark.parametrize("name", list(A.TYPES))
def test_model_narrow_is_torchs_round_to_nearest_even(name):
    dt = A.TYPES[name]
    rng = np.random.default_rng(dt)
    x = np.concatenate([rng.integers(0, 2 ** 32, size=1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32), _halfway(dt)])
    got, want = A.narrow(x, dt), _torch_narrow(x, dt)
    assert A.same(got, want, dt)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan]) and np.all(np.isnan(A.widen(got[nan], dt)))
    # the halfway points really are ties: the float32 just below goes to one pattern, the one just
    # above to the next, and the tie itself to whichever of the two is even -- both ways occur, so
    # truncation and round-half-away each differ from the model somewhere
    h = _halfway(dt)
    lo = A.narrow(np.nextafter(h, np.float32(0)), dt)
    up = A.narrow(np.nextafter(h, np.copysign(np.float32(np.inf), h)), dt)
    g = A.narrow(h, dt)
    assert np.array_equal(up, lo + 1)
    assert np.array_equal(g, np.where(lo & 1, up, lo)) and 0 < np.sum(g == lo) < h.size


def test_piece_geometry_of_the_converting_kernel():
    """tests/kernel_plan_acc32: the plain build, and once more as a stand-alone program whose host
    code is built with ASan + UBSan (nothing is preloaded)."""
    d = os.path.join(ROOT, "tests", "kernel_plan_acc32")
    subprocess.run(["make", "-s", "-C", d], check=True)
    san = os.path.join(d, "_build", "planacc32_check_san")
    flags = subprocess.run(["nm", san], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in flags and "__ubsan_handle" in flags  # really built with the sanitizers
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    for exe in (os.path.join(d, "_build", "planacc32_check"), san):
        cp = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert cp.returncode == 0, cp.stdout + cp.stderr[-3000:]
        words = cp.stdout.split()
        assert words[0] == "OK" and int(words[1]) > 50000 and int(words[3]) > 1000, cp.stdout


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "fault-tolerant_amd"), "-j8"], check=True)
    return os.path.join(ROOT, "fault-tolerant_amd", "lib", "libftar.so")


def test_symbol_is_exported_and_mapped(built, hostsim):
    for lib in (built, os.path.join(hostsim, "libftar_hostsim.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        assert any(line.split()[-1] == "ftar_allreduce_multi_acc32" and " T " in line for line in out.splitlines()), lib
    assert re.search(r"\bftar_allreduce_multi_acc32;", open(os.path.join(ROOT, "fault-tolerant_amd", "csrc", "ftar.map")).read())
    # the mover is the device layer's kernel launch, all four kernels (2 directions x 2 types)
    syms = subprocess.run(["nm", built], capture_output=True, text=True, check=True).stdout
    assert re.search(r" [Tt] fdev_gather_cvt$", syms, flags=re.M)
    assert len(set(re.findall(r"\b(\w*gather_cvt_kernel\w*)", syms))) >= 4
    # ... and a weak reference the host-sim library leaves undefined
    hs = subprocess.run(["nm", "-D", os.path.join(hostsim, "libftar_hostsim.so")], capture_output=True, text=True, check=True).stdout
    assert re.search(r" w fdev_gather_cvt$", hs, flags=re.M) and not re.search(r" [Tt] fdev_gather_cvt$", hs, flags=re.M)


def test_header_and_binding_agree(ftar):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ftar.h")).read(), flags=re.S)
    m = re.search(r"int\s+ftar_allreduce_multi_acc32\s*\(([^)]*)\)", src)
    assert m, "not declared"
    params = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert len(params) == 9 and params[7] == "float scale" and params[8] == "ftar_comm *comm", params
    assert hasattr(ftar.Comm, "allreduce_multi_acc32")
    import inspect
    sig = inspect.signature(ftar.Comm.allreduce_multi_acc32)
    assert list(sig.parameters)[1:] == ["tensors", "out", "op", "algo", "scale"]
    assert sig.parameters["scale"].default == 1.0 and sig.parameters["algo"].default == "raben"
    assert '"ftar_allreduce_multi_acc32"' in open(os.path.join(ROOT, "fault-tolerant_amd", "__init__.py")).read()
    # ftar_stats is as it was: `coalesced` last
    body = re.search(r"typedef struct\s*\{([^{}]*)\}\s*ftar_stats\s*;", src).group(1)
    assert re.findall(r"(\w+)\s*;", body)[-1] == "coalesced" == ftar.Stats._fields_[-1][0]


@pytest.fixture()
def solo(hostsim, monkeypatch):
    """The host-sim library and a one-rank comm of it."""
    monkeypatch.setenv("FTAR_HOSTSIM_TAG", f"acc32{os.getpid()}")
    monkeypatch.delenv("FTAR_LAUNCHER", raising=False)
    monkeypatch.delenv("FTAR_KILL", raising=False)
    L = ctypes.CDLL(os.path.join(hostsim, "libftar_hostsim.so"))
    L.ftar_allreduce_multi_acc32.argtypes = ACC32_ARGS
    L.ftar_init_rank.argtypes = [ctypes.POINTER(VP), ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ftar_finalize.argtypes = [VP]
    h = VP()
    assert L.ftar_init_rank(ctypes.byref(h), f"/ftar-acc32-{os.getpid()}".encode(), 0, 1, 0) == 0
    yield L, h
    L.ftar_finalize(h)


GUARD = 8


def test_hostsim_refuses_both_types_and_touches_nothing(solo):
    L, h = solo
    counts = [3, 5, 0, 2]
    ins = [np.full(c + 2 * GUARD, 0x3C00, dtype=np.uint16) for c in counts]
    outs = [np.full(c + 2 * GUARD, 0xEEEE, dtype=np.uint16) for c in counts]
    sb = (VP * 4)(*[a.ctypes.data + 2 * GUARD for a in ins])
    rb = (VP * 4)(*[a.ctypes.data + 2 * GUARD for a in outs])
    ct = (SZ * 4)(*counts)
    f = L.ftar_allreduce_multi_acc32
    for algo in (RD, RABEN):
        for dt in (16, 17):  # the host-sim device layer has neither type
            assert f(algo, sb, rb, ct, 4, dt, 0, 1.0, h) == ERR_ARG
            assert f(algo, sb, sb, ct, 4, dt, 2, 0.5, h) == ERR_ARG
        assert f(algo, sb, rb, ct, 4, 16, 0, 1.0, None) == ERR_ARG          # no comm
        assert f(algo, sb, rb, ct, 4, 1, 0, 1.0, None) == ERR_ARG
        assert f(algo, sb, rb, ct, 4, 1, 4, 1.0, h) == ERR_OP               # the op check comes first: LAND on float32
        assert f(algo, None, None, None, 0, 1, 4, float("nan"), h) == ERR_OP  # ... before every other argument
        assert f(algo, sb, rb, ct, 4, 0, 16, 1.0, h) == ERR_OP              # MAXLOC on int32
        assert f(algo, sb, rb, ct, 4, 1, 0, 1.0, h) == ERR_ARG              # float32: ftar_allreduce_multi's
        assert f(algo, sb, rb, ct, 4, 0, 0, 1.0, h) == ERR_ARG              # int32
        assert f(algo, sb, rb, ct, 4, 5, 0, 1.0, h) == ERR_ARG              # no such type
        assert f(algo, sb, rb, ct, 4, 1, 0, float("inf"), h) == ERR_ARG
    for o in outs:
        assert np.all(o == 0xEEEE)
    for a in ins:
        assert np.all(a == 0x3C00)


def test_binding_refuses_before_anything_is_called(hostsim, monkeypatch):
    import importlib.util
    import torch
    monkeypatch.setenv("FTAR_HOSTSIM_TAG", f"acc32b{os.getpid()}")
    monkeypatch.delenv("FTAR_LAUNCHER", raising=False)
    monkeypatch.delenv("FTAR_KILL", raising=False)
    spec = importlib.util.spec_from_file_location("ftar_amd_acc32_binding", os.path.join(ROOT, "fault-tolerant_amd", "__init__.py"))
    ftar = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ftar)
    ftar.use_test_library(os.path.join(hostsim, "libftar_hostsim.so"))

    class NoCall(ftar.Comm):
        def __init__(self):
            self._h = None

    c = NoCall()
    a, b = torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.float16)
    with pytest.raises(ftar.FtarError, match="one dtype"):
        c.allreduce_multi_acc32([a, b])
    with pytest.raises(ftar.FtarError, match="float16 or bfloat16"):
        c.allreduce_multi_acc32([torch.zeros(4, dtype=torch.float32)])
    with pytest.raises(ftar.FtarError, match="contiguous"):
        c.allreduce_multi_acc32([a, torch.zeros(8, dtype=torch.bfloat16)[::2]])
    with pytest.raises(ftar.FtarError, match="as many outputs"):
        c.allreduce_multi_acc32([a], out=[a, a])
    with pytest.raises(ftar.FtarError, match="size differs"):
        c.allreduce_multi_acc32([a], out=[torch.zeros(5, dtype=torch.bfloat16)])
    with pytest.raises(ftar.FtarError, match="unknown algo"):
        c.allreduce_multi_acc32([a], algo="ring")
    with pytest.raises(ftar.FtarError, match="tensors"):
        c.allreduce_multi_acc32([])
    # a valid list reaches the library, whose host-sim build has no 2-byte types: FTAR_ERR_ARG
    comm = ftar.Comm.init_rank(f"/ftar-acc32-bind-{os.getpid()}", 0, 1, 0)
    try:
        x = torch.ones(5, dtype=torch.bfloat16)
        assert comm.allreduce_multi_acc32([x], scale=0.5) == ERR_ARG and torch.equal(x, torch.ones(5, dtype=torch.bfloat16))
    finally:
        comm.finalize()
