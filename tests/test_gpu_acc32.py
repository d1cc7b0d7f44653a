"""ftar_allreduce_multi_acc32 on the GPU: the converting gather / scatter kernels and the call's
contract -- widen exactly, the plain float32 schedule on the dense concatenation, one float32
multiplication by the caller's scale, one rounding to nearest even, scatter.

Every GPU action runs in a child: tests/acc32/acc32_probe.c (built against libftar.so, every entry
in a hipMalloc'd buffer of its own, (i + offset) % 8 elements past a 16-byte boundary, with guards
on both sides), tests/acc32_worker.py (the torch binding) or bin/ftbench as the ranks of an ftrun
job, all on GPU 0.  The pytest process never opens the GPU; every child has its own timeout and a
test stops at the first child that fails.

The expectation is tests/acc32_runner.py's numpy model around the unchanged float32 oracle,
compared bit for bit, except that where the model holds a NaN the result must hold a NaN of any
payload (so the payload difference between the oracle's x86 and the GPU that test_gpu_multi.py
documents does not show here).  No other element is exempt.
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import acc32_runner as A
import fence_check as FC
import harness as H
import multi_runner as R

pytestmark = pytest.mark.gpu

LIST = R.COUNTS + R.TINY40
N = sum(LIST)
# all 65536 patterns: sizes around a vector and around a packed tile (4096 elements), an empty
# entry, 40 tiny ones, and the rest in one entry that spans twelve tiles
P1_COUNTS = [1, 3, 0, 5, 4093, 4099, 8193] + R.TINY40
P1_COUNTS = P1_COUNTS + [65536 - sum(P1_COUNTS)]


@pytest.fixture(scope="module")
def probe():
    return A.build()


def _fn(oracle, algo):
    return oracle.rabenseifner if algo == "raben" else oracle.recursive_doubling


@pytest.mark.parametrize("name", list(A.TYPES))
def test_every_bit_pattern_round_trips(probe, name):
    """p = 1, scale 1: no arithmetic, so the output is the input bit for bit (a NaN for a NaN) --
    both conversions on every pattern, subnormals included.  Four jobs: offset 0 and 1, out of place
    through Rabenseifner's entry and in place through recursive doubling's."""
    dt = A.TYPES[name]
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    nan = np.isnan(A.widen(x, dt))
    for algo, inplace, offset in (("raben", 0, 0), ("raben", 0, 1), ("rd", 1, 0), ("rd", 1, 1)):
        r = A.run_acc32(algo, [(P1_COUNTS, [x])], 1, dtype=dt, inplace=inplace, offset=offset, timeout=60)
        what = (name, algo, inplace, offset)
        assert r.returncode == 0, (what, r.stderr[-2000:])
        s = r.status[0][0]
        assert (s[R.RC], s[R.CSIZE]) == (0, 1), (what, s)
        assert s[R.INTACT] == 1, (what, "a guard or an input was written")
        assert s[R.COALESCED] == sum(1 for c in P1_COUNTS if c), (what, s)
        assert s[A.HBM] >= 12 * 65536, (what, s)  # 6 bytes per element for each of the two launches, plus the one-rank copy
        got = r.outputs[0][0]
        assert np.array_equal(got[~nan], x[~nan]), (what, np.flatnonzero((got != x) & ~nan)[:8])
        assert np.all(np.isnan(A.widen(got[nan], dt))), what


def _ties(dt):
    """(v, h): every finite pattern v whose half-ulp is representable, and that half-ulp with v's
    sign.  widen(v) + widen(h) is exact in float32 and lies halfway between v and the next
    pattern away from zero."""
    mb, bias, emax = (10, 15, 31) if dt == A.F16 else (7, 127, 255)
    v = np.arange(1 << 15, dtype=np.uint32)
    e = v >> mb
    v, e = v[(e >= 2) & (e < emax)], e[(e >= 2) & (e < emax)]  # biased exponent 2: half an ulp is the smallest subnormal
    half = np.ldexp(1.0, e.astype(np.int64) - bias - mb - 1).astype(np.float32)
    h = A.narrow(half, dt).astype(np.uint32)
    assert np.array_equal(A.widen(h.astype(np.uint16), dt), half)
    v, h = np.concatenate([v, v | 0x8000]), np.concatenate([h, h | 0x8000])
    return v.astype(np.uint16), h.astype(np.uint16)


@pytest.mark.parametrize("name", list(A.TYPES))
def test_ties_and_range(probe, oracle, name):
    """p = 2, SUM, four calls of one job.  Ties: every sum is exact in float32 and exactly halfway
    between two patterns, so nearest-even differs from truncation and from round-half-away (the
    largest ones round to inf).  Range: v + v beyond 65504 -- inf in float16 at scale 1, finite
    again at scale 0.5 -- and a block that scale 2^-12 takes into the type's subnormals."""
    dt = A.TYPES[name]
    v, h = _ties(dt)
    rng = np.random.default_rng(dt)
    big = A.narrow((rng.uniform(33000, 65504, size=N) * rng.choice([-1, 1], size=N)).astype(np.float32), dt)
    emin = -14 if dt == A.F16 else -126
    small = A.narrow((rng.uniform(1, 2, size=N) * np.exp2(emin + 12 - rng.integers(1, 8, size=N)) * rng.choice([-1, 1], size=N)).astype(np.float32), dt)
    small2 = A.narrow((rng.uniform(1, 2, size=N) * np.exp2(emin + 12 - rng.integers(1, 8, size=N))).astype(np.float32), dt)
    calls = [(LIST + [v.size - N], [v, h]), (LIST, [big, big]), (LIST, [big, big]), (LIST, [small, small2])]
    scales = [1.0, 1.0, 0.5, 2.0 ** -12]
    models = [A.model(oracle.rabenseifner, ins, dt, 0, s) for (_, ins), s in zip(calls, scales)]
    # the inputs do what the test is about (this is about the model, before anything runs)
    t = models[0][1][0]
    assert np.all((t == v) | (t == v + 1)) and np.all(t & 1 == 0) and 0 < np.sum(t == v) < v.size
    if dt == A.F16:
        assert np.all(np.isinf(A.widen(models[1][1][0], dt))) and np.all(np.isfinite(A.widen(models[2][1][0], dt)))
    sub = A.widen(models[3][1][0], dt)
    assert np.mean(np.abs(sub) < 2.0 ** emin) > 0.5 and np.any(sub != 0)
    r = A.run_acc32("raben", calls, 2, dtype=dt, op=0, scale=scales, offset=1, timeout=90)
    assert r.returncode == 0, r.stderr[-2000:]
    for k, (c, _) in enumerate(calls):
        A.check_against_model(models[k][0], models[k][1], r, k, c, dt, (name, k))


@pytest.mark.parametrize("p", [2, 4, 3, 5])
@pytest.mark.parametrize("algo", ["raben", "rd"])
def test_equals_oracle_and_plain_float32_call(probe, oracle, algo, p):
    """Both types in one job: SUM with scale 1 / p and MAX with scale 1, inputs with NaN, +-0 and
    +-inf.  Against the model; and the plain float32 entry point, run by the probe in the same job
    on the widened vector, gives after narrow(scale * .) the new call's output (same NaN rule).
    Where that plain result differs from the oracle, both hold a NaN."""
    fn = _fn(oracle, algo)
    calls, dts, ops, scales = [], [], [], []
    for dt in (A.F16, A.BF16):
        for op, scale, seed in ((0, float(np.float32(1) / np.float32(p)), 1), (2, 1.0, 2)):
            calls.append((LIST, A.specials16(oracle, p, N, dt, seed=10 * p + dt + seed)))
            dts.append(dt)
            ops.append(op)
            scales.append(scale)
    r = A.run_acc32(algo, calls, p, dtype=dts, op=ops, scale=scales, plain=True, offset=p % 2, timeout=90)
    assert r.returncode == 0, r.stderr[-2000:]
    for k, (c, ins) in enumerate(calls):
        o, want = A.model(fn, ins, dts[k], ops[k], scales[k])
        A.check_against_model(o, want, r, k, c, dts[k], (algo, p, k))
        for w in range(p):
            assert r.status[k][w][R.PLAIN_RC] == 0
            with np.errstate(over="ignore", invalid="ignore"):
                via_plain = A.narrow(np.float32(scales[k]) * r.plain[k][w], dts[k])
            assert A.same(r.outputs[k][w], via_plain, dts[k]), (algo, p, k, w, "differs from narrow(scale * plain float32 call)")
            bad = np.flatnonzero(r.plain[k][w].view(np.uint32) != o.outputs[w].view(np.uint32))
            assert np.all(np.isnan(r.plain[k][w][bad])) and np.all(np.isnan(o.outputs[w][bad])), (algo, p, k, w)


# test_gpu_multi.KILLS: per schedule the kills the existing suites use (the oracle: both recover)
# and one that dies in the first loop step, which the reference cannot recover from (MPI_Abort)
KILLS = [("raben", 5, (4, 1, 1, 1)), ("raben", 5, (3, 2, 0, 1)), ("raben", 5, (1, 1, 0, 1)),
         ("rd", 6, (1, 1, 1, 2)), ("rd", 6, (3, 1, 1, 3)), ("rd", 6, (1, 1, 0, 1))]


@pytest.mark.parametrize("algo,p,kill", KILLS, ids=[f"{a}-p{p}-{'_'.join(map(str, k))}" for a, p, k in KILLS])
def test_kills_end_as_the_oracle_says(probe, oracle, algo, p, kill):
    """bfloat16 SUM: outcome class, return code, comm size, recoveries and the survivors' bits are
    the oracle's on the widened inputs; the aborting case writes no output."""
    ins = A.specials16(oracle, p, sum(R.COUNTS), A.BF16, seed=3 * p)
    o, want = A.model(_fn(oracle, algo), ins, A.BF16, 0, 1.0, kills=[kill])
    assert o.aborted == (kill == (1, 1, 0, 1)) and (o.aborted or o.recoveries == 1)
    r = A.run_acc32(algo, [(R.COUNTS, ins)], p, dtype=A.BF16, op=0, kills=[kill], timeout=90)
    A.check_against_model(o, want, r, 0, R.COUNTS, A.BF16, (algo, p, kill))


def test_limit_regrowth_and_the_other_mover(probe, oracle):
    """nbufs = FTAR_MULTI_MAX with 1..7 elements each, inside a call sequence whose totals grow,
    shrink and grow again, with a plain ftar_allreduce_multi bfloat16 call in between (the two movers
    share the staging and the table mirror); p = 2, bfloat16 SUM, scale 0.5."""
    p, dt = 2, A.BF16
    lists = [R.TINY40, [1 + (i * 11) % 7 for i in range(1024)], [2, 2], R.COUNTS + [70001, 3], R.COUNTS, R.COUNTS]
    modes = [0, 0, 0, 0, 1, 0]
    calls = [(c, A.specials16(oracle, p, sum(c), dt, seed=40 + k)) for k, c in enumerate(lists)]
    for algo in ("raben", "rd"):
        r = A.run_acc32(algo, calls, p, dtype=dt, op=0, scale=0.5, mode=modes, offset=1, timeout=90)
        assert r.returncode == 0, r.stderr[-2000:]
        for k, (c, ins) in enumerate(calls):
            if modes[k] == 0:
                o, want = A.model(_fn(oracle, algo), ins, dt, 0, 0.5)
                A.check_against_model(o, want, r, k, c, dt, (algo, "sequence", k))
                continue
            # the 16-bit call at p = 2: one float32 addition, rounded once (no scale)
            with np.errstate(over="ignore", invalid="ignore"):
                want = A.narrow(A.widen(ins[0], dt) + A.widen(ins[1], dt), dt)
            for w in range(p):
                s = r.status[k][w]
                assert (s[R.RC], s[R.INTACT], s[R.COALESCED]) == (0, 1, sum(1 for x in c if x)), (algo, k, w, s)
                assert A.same(r.outputs[k][w], want, dt), (algo, "plain multi in between", w)


@pytest.mark.parametrize("algo", ["raben", "rd"])
def test_fence_discipline_of_an_acc32_job(probe, oracle, algo):
    """FTAR_TRACE logs of a p = 2 job through tests/fence_check.py's checker, unchanged: a small
    list (staged input, gated launches) and, twice, one above the staging limit, whose gathered
    float32 vector the peer reads in place -- the gather's stores must be released before the first
    barrier.  The second large call finds the staging vector registered with the trace from the
    first, so its gather launch shows the packed range it writes: 4 bytes per element."""
    p, dt = 2, A.BF16
    big = R.COUNTS + [300001]
    lists = [R.COUNTS, big, big]
    calls = [(c, A.specials16(oracle, p, sum(c), dt, seed=90 + k)) for k, c in enumerate(lists)]
    tmp = tempfile.mkdtemp(prefix="ftar_acc32_fence_")
    try:
        r = A.run_acc32(algo, calls, p, dtype=dt, op=0, scale=0.5, env_extra={"FTAR_TRACE": os.path.join(tmp, "t")}, timeout=90)
        assert r.returncode == 0, r.stderr[-2000:]
        for k, (c, ins) in enumerate(calls):
            o, want = A.model(_fn(oracle, algo), ins, dt, 0, 0.5)
            A.check_against_model(o, want, r, k, c, dt, (algo, "traced", k))
        logs = FC.load(os.path.join(tmp, "t"))
        assert sorted(logs) == list(range(p))
        rep = FC.check(logs)
        assert rep.ok, (rep.release[:5], rep.acquire[:5])
        assert rep.reads_checked > 0
        for w in range(p):
            text = open(os.path.join(tmp, f"t.{w}")).read()
            launches = [ln for ln in text.splitlines() if ln.startswith("L ") and " eng=k " in ln]
            assert len(launches) >= 6  # a gather and a scatter per call, and the schedule's own
            assert any(re.search(rf" w={w}:U\d+:\d+:{4 * sum(big)},", ln) for ln in launches), (w, "the gather's packed range")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_torch_binding(oracle):
    """Comm.allreduce_multi_acc32 on lists of torch tensors, p = 2: bfloat16 in place with SUM and
    scale 0.5, float16 out of place with MAX and algo="rd"."""
    p, counts = 2, [1, 3, 0, 5, 4093, 2]
    jobs = [(A.BF16, oracle.rabenseifner, 0, 0.5), (A.F16, oracle.recursive_doubling, 2, 1.0)]
    ins = [A.specials16(oracle, p, sum(counts), dt, seed=77 + dt) for dt, _, _, _ in jobs]
    tmp = tempfile.mkdtemp(prefix="ftar_acc32_torch_")
    try:
        for k, per_rank in enumerate(ins):
            for r, x in enumerate(per_rank):
                x.tofile(os.path.join(tmp, f"in_{r}_{k}.bin"))
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, MULTI_COUNTS=",".join(map(str, counts)))
        env.pop("FTAR_KILL", None)
        cp = subprocess.run([os.path.join(H.PKG, "bin", "ftrun"), "-np", str(p), "--devmap", "0,0", sys.executable, "-u",
                             os.path.join(H.ROOT, "tests", "acc32_worker.py")], env=env, capture_output=True, text=True,
                            timeout=120)
        assert cp.returncode == 0, cp.stderr[-3000:]
        nonempty = sum(1 for c in counts if c)
        for k, (dt, fn, op, scale) in enumerate(jobs):
            _, want = A.model(fn, ins[k], dt, op, scale)
            for w in range(p):
                st = tuple(int(v) for v in open(os.path.join(tmp, f"status_{w}_{k}.txt")).read().split())
                assert st == (0, nonempty, 1), (w, k, st)
                got = np.fromfile(os.path.join(tmp, f"out_{w}_{k}.bin"), dtype=np.uint16)
                assert A.same(got, want[w], dt), (w, k)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_ftbench_acc32():
    """bin/ftbench with FTBENCH_MULTI=7 FTBENCH_ACC32=1 on both types and both schedules, p = 2: its
    own check (every element its exact sum) and its output line are the plain job's."""
    env = dict(os.environ, FTBENCH_MULTI="7", FTBENCH_ACC32="1", FTBENCH_PATTERN="1")
    env.pop("FTAR_KILL", None)
    for tn in ("bf16", "f16"):
        for algo in ("raben", "rd"):
            cp = subprocess.run([os.path.join(H.PKG, "bin", "ftrun"), "-np", "2", "--devmap", "0,0",
                                 os.path.join(H.PKG, "bin", "ftbench"), algo, "70001", "2", tn], env=env, capture_output=True,
                                text=True, timeout=60)
            assert cp.returncode == 0, (tn, algo, cp.stderr[-2000:])
            lines = [json.loads(ln) for ln in cp.stdout.splitlines() if ln.startswith("{")]
            assert sorted(ln["rank"] for ln in lines) == [0, 1]
            for ln in lines:
                assert all(c["rc"] == 0 and c["uniform"] and c["comm_size"] == 2 for c in ln["calls"]), (tn, algo, ln)
                # float32 staging: 6 bytes per element for each mover, and the schedule's 4-byte traffic
                assert all(c["hbm_bytes"] >= 12 * 70001 for c in ln["calls"]), (tn, algo, ln)
