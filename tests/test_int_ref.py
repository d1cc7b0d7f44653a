"""The plain reference behind the integer types' GPU checks (tests/int_types/int_ref.h), pinned on
the CPU, with the self-test of the GPU checker's inputs and the planner walk.

tests/int_types/ref_check is a host program (no HIP call): `apply` runs the reference over operand
files, `selftest` generates the inputs of every case of int_check and asserts that they tell a
right kernel from the wrong ones a packed or SWAR implementation can be (signedness of the compare
swapped, saturating instead of wrapping, a carry leaking into the neighbouring element, a product's
upper half kept, a logical result other than 0 / 1), `planwalk` replays gather_piece at 1- and
2-byte elements.  All three also run in a build with ASan + UBSan.  The planners (plan_segments,
plan_tree, plan_tree_batch) at those sizes are walked by tests/kernel_plan.

References here: numpy's fixed-width integer arithmetic (int_model.combine, overflow warnings off)
* 8-bit: all 65 536 operand pairs x 10 ops x both signednesses;
* 16-bit: every pattern against 48 partners (16 specials as `in`, the same as `inout`, 16
  rotations), the rule test_kernel_ref.py uses for the 2-byte floats;
* 32 / 64-bit unsigned: specials around 0, 2^31, 2^32 - 1, 2^63, 2^64 - 1, plus random.
And the value maps of the GPU kill tests commute with every op (int_model.to_oracle / from_oracle).
"""
import fcntl
import os
import subprocess
import tempfile

import numpy as np
import pytest

import int_model as I
from plan_checks import run_planwalk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "int_types")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # (the HIP runtime's start-up allocations: hipcc links it)


@pytest.fixture(scope="module")
def ref_check():
    """(plain, sanitized) builds of the program: header only, nothing of the product is linked."""
    os.makedirs(os.path.join(DIR, "_build"), exist_ok=True)
    with open(os.path.join(DIR, "_build", ".ref.lock"), "w") as lk:  # one build at a time (pytest-xdist workers)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", DIR, "_build/ref_check", "_build/ref_check_san"], check=True)
    plain, san = os.path.join(DIR, "_build", "ref_check"), os.path.join(DIR, "_build", "ref_check_san")
    syms = subprocess.run(["nm", san], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms  # really built with the sanitizers
    return plain, san


def apply(exe, tmp, dt, op, inout, in_, env=None):
    fi, fio, fo = (os.path.join(tmp, n) for n in ("in.bin", "inout.bin", "out.bin"))
    I.raw(in_).tofile(fi)
    I.raw(inout).tofile(fio)
    cp = subprocess.run([exe, "apply", str(dt), str(op), fi, fio, fo], capture_output=True, text=True, timeout=300, env=env)
    assert cp.returncode == 0, cp.stdout + cp.stderr[-3000:]
    return np.fromfile(fo, dtype=I.NP[dt])


@pytest.mark.parametrize("dt", I.TYPES, ids=[I.NAMES[t] for t in I.TYPES])
def test_reference_matches_numpy(ref_check, dt):
    x, y = I.operands(dt)
    assert x.size == {8: 1 << 16, 16: 48 << 16}.get(8 * x.itemsize, x.size)
    with tempfile.TemporaryDirectory(prefix="ftar_intref_") as tmp:
        for op in I.OPS:
            want = I.combine(op)(x, y)
            got = apply(ref_check[0], tmp, dt, op, x, y)
            assert got.dtype == want.dtype and got.shape == want.shape
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (I.NAMES[dt], I.OP_NAMES[op], bad[:8], x[bad[:8]], y[bad[:8]], got[bad[:8]], want[bad[:8]])


def test_numpy_model_is_what_the_header_says():
    """The model itself on the cases the header names: wrap modulo 2^w, the type's own signedness,
    0 / 1."""
    i8, u8, u16 = (lambda *v: np.array(v, dtype=np.int8)), (lambda *v: np.array(v, dtype=np.uint8)), (lambda *v: np.array(v, dtype=np.uint16))
    assert I.combine(I.SUM)(i8(127, -128), i8(1, -1)).tolist() == [-128, 127]
    assert I.combine(I.SUM)(u8(255), u8(1)).tolist() == [0]
    assert I.combine(I.PROD)(u16(65535), u16(65535)).tolist() == [1]
    assert I.combine(I.PROD)(i8(-128), i8(-1)).tolist() == [-128]
    assert I.combine(I.MAX)(i8(-128), i8(127)).tolist() == [127] and I.combine(I.MAX)(u8(0x80), u8(0x7F)).tolist() == [0x80]
    assert I.combine(I.MIN)(i8(-128), i8(127)).tolist() == [-128] and I.combine(I.MIN)(u8(0x80), u8(0x7F)).tolist() == [0x7F]
    assert I.combine(I.LAND)(u8(2, 2), u8(4, 0)).tolist() == [1, 0] and I.combine(I.LXOR)(u8(2, 2), u8(4, 0)).tolist() == [0, 1]
    assert I.combine(I.LOR)(i8(-128, 0), i8(0, 0)).tolist() == [1, 0]
    assert I.combine(I.BXOR)(u16(0xFF00), u16(0x0FF0)).tolist() == [0xF0F0]


def test_inputs_tell_a_wrong_kernel_from_a_right_one(ref_check):
    for exe, env in ((ref_check[0], None), (ref_check[1], SAN_ENV)):
        cp = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=300, env=env)
        assert cp.returncode == 0, cp.stdout[-3000:] + cp.stderr[-3000:]
        assert cp.stdout.startswith("selftest OK ") and int(cp.stdout.split()[2]) >= 100, cp.stdout


def test_plans_cover_one_and_two_byte_elements(ref_check):
    """The planners at esize 1 and 2 (tests/kernel_plan) and the gather walk that stays here: at
    least the cases of the one walk these types came with (367488 + 91916 planner cases, 20882
    gather cases)."""
    assert run_planwalk(1) >= 367488
    assert run_planwalk(2) >= 91916
    for exe, env in ((ref_check[0], None), (ref_check[1], SAN_ENV)):
        cp = subprocess.run([exe, "planwalk"], capture_output=True, text=True, timeout=300, env=env)
        assert cp.returncode == 0, cp.stdout[-3000:] + cp.stderr[-3000:]
        assert cp.stdout.startswith("planwalk OK ") and int(cp.stdout.split()[2]) >= 20882, cp.stdout


def test_reference_under_sanitizers(ref_check):
    with tempfile.TemporaryDirectory(prefix="ftar_intref_") as tmp:
        for dt in I.TYPES:
            x, y = I.operands(dt)
            x, y = x[:1 << 16], y[:1 << 16]
            for op in (I.SUM, I.PROD, I.MAX, I.LXOR):
                assert np.array_equal(apply(ref_check[1], tmp, dt, op, x, y, SAN_ENV), apply(ref_check[0], tmp, dt, op, x, y))


@pytest.mark.parametrize("dt", I.TYPES, ids=[I.NAMES[t] for t in I.TYPES])
def test_oracle_value_maps_commute(dt):
    """from_oracle(int64 op on to_oracle(x), to_oracle(y)) == x op y for every op, pairwise: what
    lets the unchanged oracle, which knows int64, check a schedule on these types.  The int64 side
    is int_model.combine on int64 arrays -- numpy's int64 arithmetic standing in for the oracle's,
    which test_oracle.py pins.  For the 16-bit types PROD also folds nine vectors of the kill tests'
    own factors (magnitude 20 .. 100): the exact product fits int64 and is far past 16 bits."""
    if dt in (I.INT16, I.UINT16):
        rng = np.random.default_rng(9)
        vs = [(rng.integers(20, 101, size=4099) * (rng.choice([-1, 1], size=4099) if dt == I.INT16 else 1)).astype(I.NP[dt])
              for _ in range(9)]
        acc = I.to_oracle(vs[0], dt, I.PROD)
        for v in vs[1:]:
            acc = I.int64_combine(I.PROD)(acc, I.to_oracle(v, dt, I.PROD))
        exact = [int(np.prod([int(v[i]) for v in vs], dtype=object)) for i in range(64)]
        assert all(int(acc[i]) == exact[i] and abs(exact[i]) > 1 << 16 for i in range(64))  # the int64 fold never wrapped
        assert np.array_equal(I.from_oracle(acc, dt, I.PROD), I.reduce_ranks(vs, I.PROD))
    x, y = I.operands(dt)
    for op in I.OPS:
        want = I.combine(op)(x, y)
        got = I.from_oracle(I.int64_combine(op)(I.to_oracle(x, dt, op), I.to_oracle(y, dt, op)), dt, op)
        assert got.dtype == want.dtype
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (I.NAMES[dt], I.OP_NAMES[op], x[bad[:4]], y[bad[:4]], got[bad[:4]], want[bad[:4]])
