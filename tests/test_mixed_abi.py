"""ftar_allreduce_multi_mixed without a GPU.

* the numpy model the GPU tests compare against (tests/mixed_runner.py) widens and narrows per entry
  with acc32_runner's conversions, which tests/test_acc32_abi.py proves against torch;
* the mixed kernel's tile -> entry -> piece walk over tables of mixed types (tests/kernel_plan_mixed:
  a host program, run plain and built with ASan + UBSan as a stand-alone binary; nothing is
  preloaded);
* the symbol is exported by the product library and the host-sim library and listed in
  csrc/ftar.map; the device hook fdev_gather_mix is the product's kernel launch and a weak
  undefined reference in host-sim; header and binding agree; ftar_stats still ends in `coalesced`;
* on the host-sim library, which has no mixed mover, the op check comes before every other
  argument and a valid list returns FTAR_ERR_ARG with nothing touched;
* the binding refuses what it must before anything is called.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import acc32_runner as A
import mixed_runner as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
MIXED_ARGS = [ctypes.c_int, ctypes.POINTER(VP), ctypes.POINTER(VP), ctypes.POINTER(SZ), ctypes.POINTER(ctypes.c_int),
              ctypes.c_int, ctypes.c_int, ctypes.c_float, VP]
RD, RABEN = 0, 1
ERR_OP, ERR_ARG = 9, 13


def test_model_widens_and_narrows_per_entry():
    counts, types = [3, 0, 2, 4, 1], [M.BF16, M.F32, M.F32, M.F16, M.BF16]
    f = np.array([1.5, -0.0, 3.0e38, 1.0 + 2.0 ** -20, -2.0 ** -140, 65520.0, 2.0 ** -25, -1.0, np.nan, 0.3], dtype=np.float32)
    raw = M.narrow_list(f, counts, types)
    assert raw.size == M.nbytes(counts, types) == 3 * 2 + 2 * 4 + 4 * 2 + 2
    assert np.array_equal(raw[:6].view(np.uint16), A.narrow(f[:3], A.BF16))
    assert np.array_equal(raw[6:14].view(np.float32).view(np.uint32), f[3:5].view(np.uint32))  # a float32 entry: copied
    assert np.array_equal(raw[14:22].view(np.uint16), A.narrow(f[5:9], A.F16))
    w = M.widen_list(raw, counts, types)
    assert np.array_equal(w[3:5].view(np.uint32), f[3:5].view(np.uint32)) and np.isinf(w[5]) and np.isnan(w[8])
    assert M.same(raw, M.narrow_list(w, counts, types), counts, types)
    assert M.nan_share(raw, counts, types) == 0.1


def test_piece_geometry_of_the_mixed_kernel():
    """tests/kernel_plan_mixed: the plain build, and once more as a stand-alone program whose host
    code is built with ASan + UBSan (nothing is preloaded)."""
    d = os.path.join(ROOT, "tests", "kernel_plan_mixed")
    subprocess.run(["make", "-s", "-C", d], check=True)
    san = os.path.join(d, "_build", "planmixed_check_san")
    flags = subprocess.run(["nm", san], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in flags and "__ubsan_handle" in flags  # really built with the sanitizers
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    for exe in (os.path.join(d, "_build", "planmixed_check"), san):
        cp = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert cp.returncode == 0, cp.stdout + cp.stderr[-3000:]
        words = cp.stdout.split()
        assert words[0] == "OK" and int(words[1]) > 50000 and int(words[3]) > 1000 and int(words[6]) > 1000, cp.stdout


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "fault-tolerant_amd"), "-j8"], check=True)
    return os.path.join(ROOT, "fault-tolerant_amd", "lib", "libftar.so")


def test_symbol_is_exported_and_mapped(built, hostsim):
    for lib in (built, os.path.join(hostsim, "libftar_hostsim.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        assert any(line.split()[-1] == "ftar_allreduce_multi_mixed" and " T " in line for line in out.splitlines()), lib
    assert re.search(r"\bftar_allreduce_multi_mixed;", open(os.path.join(ROOT, "fault-tolerant_amd", "csrc", "ftar.map")).read())
    # the mover is the device layer's kernel launch, one kernel per direction
    syms = subprocess.run(["nm", built], capture_output=True, text=True, check=True).stdout
    assert re.search(r" [Tt] fdev_gather_mix$", syms, flags=re.M)
    assert len(set(re.findall(r"\b(\w*gather_mix_kernel\w*)", syms))) >= 2
    # ... and a weak reference the host-sim library leaves undefined
    hs = subprocess.run(["nm", "-D", os.path.join(hostsim, "libftar_hostsim.so")], capture_output=True, text=True, check=True).stdout
    assert re.search(r" w fdev_gather_mix$", hs, flags=re.M) and not re.search(r" [Tt] fdev_gather_mix$", hs, flags=re.M)


def test_header_and_binding_agree(ftar):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ftar.h")).read(), flags=re.S)
    m = re.search(r"int\s+ftar_allreduce_multi_mixed\s*\(([^)]*)\)", src)
    assert m, "not declared"
    params = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert params == ["ftar_algo algo", "const void *const *sbufs", "void *const *rbufs", "const size_t *counts",
                      "const ftar_dtype *dtypes", "int nbufs", "ftar_op op", "float scale", "ftar_comm *comm"], params
    sig = inspect.signature(ftar.Comm.allreduce_multi_mixed)
    assert list(sig.parameters)[1:] == ["tensors", "out", "op", "algo", "scale"]
    assert sig.parameters["scale"].default == 1.0 and sig.parameters["algo"].default == "raben" and sig.parameters["out"].default is None
    fn = ftar.lib().ftar_allreduce_multi_mixed
    assert len(fn.argtypes) == 9 and fn.argtypes[4] == ctypes.POINTER(ctypes.c_int) and fn.argtypes[7] == ctypes.c_float
    # ftar_stats is as it was: `coalesced` last
    body = re.search(r"typedef struct\s*\{([^{}]*)\}\s*ftar_stats\s*;", src).group(1)
    assert re.findall(r"(\w+)\s*;", body)[-1] == "coalesced" == ftar.Stats._fields_[-1][0]


@pytest.fixture()
def solo(hostsim, monkeypatch):
    """The host-sim library and a one-rank comm of it."""
    monkeypatch.setenv("FTAR_HOSTSIM_TAG", f"mixed{os.getpid()}")
    monkeypatch.delenv("FTAR_LAUNCHER", raising=False)
    monkeypatch.delenv("FTAR_KILL", raising=False)
    L = ctypes.CDLL(os.path.join(hostsim, "libftar_hostsim.so"))
    L.ftar_allreduce_multi_mixed.argtypes = MIXED_ARGS
    L.ftar_init_rank.argtypes = [ctypes.POINTER(VP), ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ftar_finalize.argtypes = [VP]
    h = VP()
    assert L.ftar_init_rank(ctypes.byref(h), f"/ftar-mixed-{os.getpid()}".encode(), 0, 1, 0) == 0
    yield L, h
    L.ftar_finalize(h)


GUARD = 8


def test_hostsim_checks_the_op_first_and_touches_nothing(solo):
    L, h = solo
    counts, types = [3, 5, 0, 2], [17, 1, 99, 16]
    ins = [np.full(c + 2 * GUARD, 0x3C003C00, dtype=np.uint32) for c in counts]
    outs = [np.full(c + 2 * GUARD, 0xEEEEEEEE, dtype=np.uint32) for c in counts]
    sb = (VP * 4)(*[a.ctypes.data + 4 * GUARD for a in ins])
    rb = (VP * 4)(*[a.ctypes.data + 4 * GUARD for a in outs])
    ct, ty = (SZ * 4)(*counts), (ctypes.c_int * 4)(*types)
    f = L.ftar_allreduce_multi_mixed
    for algo in (RD, RABEN):
        assert f(algo, sb, rb, ct, ty, 4, 0, 1.0, None) == ERR_ARG                    # no comm
        assert f(algo, sb, rb, ct, ty, 4, 4, 1.0, None) == ERR_ARG                    # ... before the op
        for op in (4, 16):  # LAND, MAXLOC: the op check comes before every other argument
            assert f(algo, sb, rb, ct, ty, 4, op, 1.0, h) == ERR_OP
            assert f(algo, None, None, None, None, 0, op, float("nan"), h) == ERR_OP
        assert f(algo, sb, rb, ct, ty, 4, 0, 1.0, h) == ERR_ARG                       # a valid list: no mover in this build
        assert f(algo, sb, sb, ct, ty, 4, 2, 0.5, h) == ERR_ARG
        assert f(algo, sb, rb, ct, None, 4, 0, 1.0, h) == ERR_ARG
        assert f(algo, sb, rb, ct, ty, 4, 0, float("inf"), h) == ERR_ARG
    for o in outs:
        assert np.all(o == 0xEEEEEEEE)
    for a in ins:
        assert np.all(a == 0x3C003C00)


def test_binding_refuses_before_anything_is_called(hostsim, monkeypatch):
    import importlib.util
    import torch
    monkeypatch.setenv("FTAR_HOSTSIM_TAG", f"mixedb{os.getpid()}")
    monkeypatch.delenv("FTAR_LAUNCHER", raising=False)
    monkeypatch.delenv("FTAR_KILL", raising=False)
    spec = importlib.util.spec_from_file_location("ftar_amd_mixed_binding", os.path.join(ROOT, "fault-tolerant_amd", "__init__.py"))
    ftar = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ftar)
    ftar.use_test_library(os.path.join(hostsim, "libftar_hostsim.so"))

    class NoCall(ftar.Comm):
        def __init__(self):
            self._h = None

    c = NoCall()
    a, b, f = torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.float16), torch.zeros(4, dtype=torch.float32)
    with pytest.raises(ftar.FtarError, match="float16, bfloat16 or float32"):
        c.allreduce_multi_mixed([a, torch.zeros(4, dtype=torch.int32), f])
    with pytest.raises(ftar.FtarError, match="contiguous"):
        c.allreduce_multi_mixed([a, torch.zeros(8, dtype=torch.float32)[::2], b])
    with pytest.raises(ftar.FtarError, match="as many outputs"):
        c.allreduce_multi_mixed([a], out=[a, a])
    with pytest.raises(ftar.FtarError, match="dtype differs"):
        c.allreduce_multi_mixed([a, f], out=[a, b])
    with pytest.raises(ftar.FtarError, match="size differs"):
        c.allreduce_multi_mixed([a, f], out=[a, torch.zeros(5, dtype=torch.float32)])
    with pytest.raises(ftar.FtarError, match="unknown algo"):
        c.allreduce_multi_mixed([a, f], algo="ring")
    with pytest.raises(ftar.FtarError, match="tensors"):
        c.allreduce_multi_mixed([])
    # a valid mixed list reaches the library, whose host-sim build has no mover: FTAR_ERR_ARG
    comm = ftar.Comm.init_rank(f"/ftar-mixed-bind-{os.getpid()}", 0, 1, 0)
    try:
        x, y = torch.ones(5, dtype=torch.bfloat16), torch.ones(3, dtype=torch.float32)
        assert comm.allreduce_multi_mixed([x, y], scale=0.5) == ERR_ARG
        assert torch.equal(x, torch.ones(5, dtype=torch.bfloat16)) and torch.equal(y, torch.ones(3, dtype=torch.float32))
    finally:
        comm.finalize()
