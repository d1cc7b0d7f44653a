"""The plain reference behind tree_check's and seg_check's `types` matrices, gather_check's
converting mode and lds_check (tests/kernel_gpu/ref_types.h), pinned on the CPU, and the self-test
of those matrices' inputs.

tests/kernel_gpu/ref_check is a host program (no HIP call): `apply` runs the reference over
operand files, `narrow` its float32 -> 16-bit conversion, `selftest` generates the inputs of every
GPU case and asserts that they can tell a wrong kernel from a right one (a wrong rounding, flushed
subnormals, swapped operands, a fused multiply-convert, a float32 entry of a mixed list not scaled)
and that the movers' tables -- plain, converting and mixed -- reach what
they are built to reach (the conditions are listed in ref_check.cpp).  `apply` and `selftest` also
run in a build with ASan + UBSan.

References here
* float16 / bfloat16: torch CPU arithmetic in the element type (test_gpu_half.pair), on every
  16-bit pattern against 48 partners: 16 special values as `in`, the same as `inout`, and 16
  rotations of the pattern table;
* pair types: include/ftar.h's rule in numpy on structured arrays (test_gpu_pair.loc), on
  test_gpu_pair's special and random pairs.
"""
import fcntl
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_gpu_half import SUM, PROD, MAX, MIN, TD, bits, pair, to_f32
from test_gpu_pair import MAXLOC, MINLOC, ST, fill_padding, loc, random_pairs, raw, special_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "kernel_gpu")
DTYPE = {"f16": 16, "bf16": 17, "float_int": 32, "2int": 33, "double_int": 34}


@pytest.fixture(scope="module")
def ref_check(oracle):
    """(plain, sanitized) builds of the program; the oracle library they pass the old types to
    is built by the `oracle` fixture."""
    os.makedirs(os.path.join(DIR, "_build"), exist_ok=True)
    with open(os.path.join(DIR, "_build", ".ref.lock"), "w") as lk:  # one build at a time (pytest-xdist workers)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", DIR, "ref"], check=True)
    plain, san = os.path.join(DIR, "_build", "ref_check"), os.path.join(DIR, "_build", "ref_check_san")
    syms = subprocess.run(["nm", san], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms  # really built with the sanitizers
    return plain, san


def apply(exe, tmp, dtype, op, inout, in_):
    """inout <op> in over raw byte buffers, by the program."""
    fi, fio, fo = (os.path.join(tmp, n) for n in ("in.bin", "inout.bin", "out.bin"))
    raw(in_).tofile(fi)
    raw(inout).tofile(fio)
    cp = subprocess.run([exe, "apply", str(DTYPE[dtype]), str(op), fi, fio, fo], capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stdout + cp.stderr[-3000:]
    return np.fromfile(fo, dtype=np.uint8)


def half_operands(name):
    """(inout, in): every 16-bit pattern against 48 partners."""
    import torch
    fi = torch.finfo(TD[name])
    sub = fi.smallest_normal * fi.eps  # the smallest subnormal
    inf, nan = float("inf"), float("nan")
    sp = bits(torch.tensor([0.0, -0.0, sub, -sub, 1.0, -1.0, fi.max, -fi.max, inf, -inf, nan, fi.smallest_normal,
                            fi.eps / 2, 0.5, 1.5, 2.0], dtype=torch.float64).to(TD[name]))
    assert sp.size == 16 and (sp[2], sp[3]) == (0x0001, 0x8001) and sp[8] == (0x7C00 if name == "f16" else 0x7F80)
    pat = np.arange(1 << 16, dtype=np.uint16)
    xs, ys = [], []
    for s in sp:
        const = np.full(pat.size, s, dtype=np.uint16)
        xs += [pat, const]
        ys += [const, pat]
    for k in range(16):
        xs.append(pat)
        ys.append(np.roll(pat, 4099 * (k + 1) + (1 << 11) * k))
    return np.concatenate(xs), np.concatenate(ys)


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_reference_matches_torch_on_every_pattern(ref_check, name):
    """SUM and PROD: the correctly rounded result bit for bit, NaN where torch has a NaN.  MAX and
    MIN: the chosen operand's own bits, NaN payloads included."""
    x, y = half_operands(name)
    assert x.size == 48 * (1 << 16)
    with tempfile.TemporaryDirectory(prefix="ftar_ref_") as tmp:
        for op in (SUM, PROD, MAX, MIN):
            want = pair(name, op)(x, y)
            got = apply(ref_check[0], tmp, name, op, x, y).view(np.uint16)
            assert got.shape == want.shape
            if op in (SUM, PROD):
                nan_w, nan_g = np.isnan(to_f32(want, name)), np.isnan(to_f32(got, name))
                assert np.array_equal(nan_w, nan_g), (name, op, np.flatnonzero(nan_w != nan_g)[:8])
                bad = np.flatnonzero((got != want) & ~nan_w)
            else:
                bad = np.flatnonzero(got != want)
            assert bad.size == 0, (name, op, bad[:8], x[bad[:8]], y[bad[:8]], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("name", ["float_int", "2int", "double_int"])
def test_reference_matches_the_header_rule_on_pairs(ref_check, name):
    rng = np.random.default_rng(77)
    sx, sy = special_pairs(name)
    x = np.concatenate([fill_padding(sx, rng), random_pairs(rng, 20011, name)])
    y = np.concatenate([fill_padding(sy, rng), random_pairs(rng, 20011, name)])
    with tempfile.TemporaryDirectory(prefix="ftar_ref_") as tmp:
        for op in (MAXLOC, MINLOC):
            want = raw(loc(op)(x, y))
            got = apply(ref_check[0], tmp, name, op, x, y)
            bad = np.flatnonzero((got.reshape(x.size, -1) != want.reshape(x.size, -1)).any(axis=1))
            assert bad.size == 0, (name, op, bad[:8], x[bad[:8]], y[bad[:8]])


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_narrowing_reference_matches_numpy(ref_check, name):
    """`ref_check narrow` (encode16 of a float32: the reference of the converting scatter) against
    acc32_runner.narrow (numpy's float16 conversion / the bfloat16 bit formula) on every 16-bit
    pattern widened and moved by 0, 1, half a gap - 1, half a gap and half a gap + 1 ulps of float32
    either way: the values themselves, their neighbours, and every tie with its two sides.  Bit for
    bit, a NaN where numpy has one."""
    import acc32_runner as A
    dt = DTYPE[name]
    pat = np.arange(1 << 16, dtype=np.uint16)
    wide = A.widen(pat, dt).view(np.uint32).astype(np.int64)
    half = 1 << (23 - (10 if name == "f16" else 7) - 1)  # half the gap of two neighbours, in float32 ulps (normal range)
    steps = [0, 1, half - 1, half, half + 1]
    moved = np.concatenate([wide + s for s in steps] + [wide - s for s in steps[1:]])
    moved = moved[(moved >= 0) & (moved < 1 << 32)].astype(np.uint32)
    if name == "f16":  # float16's subnormals and the range below them: the gap there is 2^-24 whatever the exponent
        tiny = np.arange(1 << 11, dtype=np.float64) * 2.0 ** -25  # every subnormal, every tie between two
        tiny = np.concatenate([tiny, -tiny]).astype(np.float32).view(np.uint32).astype(np.int64)
        moved = np.concatenate([moved, (tiny[:, None] + np.array([-1, 0, 1])).ravel().clip(0, (1 << 32) - 1).astype(np.uint32)])
    f = moved.view(np.float32)
    want = A.narrow(f, dt)
    with tempfile.TemporaryDirectory(prefix="ftar_ref_") as tmp:
        fi, fo = os.path.join(tmp, "f32.bin"), os.path.join(tmp, "h16.bin")
        f.tofile(fi)
        cp = subprocess.run([ref_check[0], "narrow", str(dt), fi, fo], capture_output=True, text=True, timeout=300)
        assert cp.returncode == 0, cp.stdout + cp.stderr[-3000:]
        got = np.fromfile(fo, dtype=np.uint16)
    assert got.shape == want.shape
    nan_w, nan_g = np.isnan(A.widen(want, dt)), np.isnan(A.widen(got, dt))
    assert np.array_equal(nan_w, np.isnan(f)) and np.array_equal(nan_w, nan_g)
    bad = np.flatnonzero((got != want) & ~nan_w)
    assert bad.size == 0, (name, bad[:8], moved[bad[:8]], got[bad[:8]], want[bad[:8]])


def test_inputs_tell_a_wrong_kernel_from_a_right_one(ref_check):
    """ref_check selftest: the conditions on the inputs of every case of the GPU matrices -- the
    tree and segment checkers' (wrong roundings, swapped operands), and those of gather_check and
    lds_check: the movers' tables replayed with the product's host functions and every unit, path,
    threshold, tile-edge exit and converting class counted non-zero; every converting scatter case
    telling a wrong rounding, flushed subnormals and a fused multiply-convert from the contract;
    -0 and half-infinity NaNs present; the NaN and finite shares; the LDS reduce's operand roles
    visible in the full tiles and in the ragged rest.  The mixed tables of `gather_check mix`
    replayed by the entry's own type: for each of float16, bfloat16 and float32 a workgroup's piece,
    a small piece on each of the four waves, a tile ending inside an entry and at an entry's end
    with each other type behind it, pieces in a workgroup's later tiles, pieces of 1020 / 1024 /
    1028 packed bytes; all 9 ordered pairs of neighbouring types in one tile; every converting class
    per 2-byte type; float32 vector pieces with heads of 1, 2 and 3 words, pieces that are not,
    the unrolled loop and its remainder, nvec = 1023 and 1024, word loops at 64 and 256 threads; a
    pinned table and one of 1024 entries.  Per mixed scatter case the converting conditions on the
    2-byte elements, and on the float32 elements a flushed subnormal product and a missing scale
    seen; over the matrix both, and a +0 for a -0 product, seen in a word and in a 16-byte vector,
    and a signalling NaN to gather in both."""
    cp = subprocess.run([ref_check[0], "selftest"], capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stdout[-3000:] + cp.stderr[-3000:]
    assert cp.stdout.rstrip().endswith("selftest: 0 failed"), cp.stdout[-3000:]
    print(cp.stdout)


def test_reference_under_sanitizers(ref_check):
    """The same program built with ASan + UBSan: the reference over operands that reach every
    branch of the rounding (specials against every pattern), and the whole self-test -- the movers'
    table generators, layouts and replay (gen_movers.h), those of the mixed tables included."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    pat = np.arange(1 << 16, dtype=np.uint16)
    with tempfile.TemporaryDirectory(prefix="ftar_ref_") as tmp:
        for name in ("f16", "bf16"):
            for op in (SUM, PROD, MAX, MIN):
                y = np.roll(pat, 4099 + op)
                plain = apply(ref_check[0], tmp, name, op, pat, y)
                fi, fio, fo = (os.path.join(tmp, n) for n in ("in.bin", "inout.bin", "out_san.bin"))
                cp = subprocess.run([ref_check[1], "apply", str(DTYPE[name]), str(op), fi, fio, fo], capture_output=True,
                                    text=True, timeout=300, env=env)
                assert cp.returncode == 0, cp.stdout + cp.stderr[-3000:]
                assert np.array_equal(np.fromfile(fo, dtype=np.uint8), plain)
        rng = np.random.default_rng(5)
        for name in ST:
            x, y = random_pairs(rng, 4099, name), random_pairs(rng, 4099, name)
            plain = apply(ref_check[0], tmp, name, MAXLOC, x, y)
            assert np.array_equal(apply(ref_check[1], tmp, name, MAXLOC, x, y), plain)
    cp = subprocess.run([ref_check[1], "selftest"], capture_output=True, text=True, timeout=900, env=env)
    assert cp.returncode == 0, cp.stdout[-3000:] + cp.stderr[-3000:]
    assert cp.stdout.rstrip().endswith("selftest: 0 failed"), cp.stdout[-3000:]
