"""ftar_allreduce_multi_mixed on the GPU: the mixed gather / scatter kernel and the call's contract
-- widen every entry by its own type, the plain float32 schedule on the dense concatenation, one
float32 multiplication by the caller's scale, a float32 entry stores the product and a 2-byte entry
the product rounded once to nearest even, scatter.

Every GPU action runs in a child: tests/mixed/mixed_probe.c (built against libftar.so, every entry
in a hipMalloc'd buffer of its own, (i + offset) % 8 elements past a 16-byte boundary, with guards
on both sides), tests/mixed_worker.py (the torch binding) or bin/ftbench as the ranks of an ftrun
job, all on GPU 0.  The pytest process never opens the GPU; every child has its own timeout and a
test stops at the first child that fails.

The expectation is tests/mixed_runner.py's numpy model around the unchanged float32 oracle,
compared bit for bit, except that where the model holds a NaN the result must hold a NaN of any
payload.  No other element is exempt, and every test asserts on the model, before a GPU child
starts, that NaN elements are at most a quarter of every compared vector.
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
import mixed_runner as M
import multi_runner as R
from test_gpu_acc32 import KILLS as ACC32_KILLS, _ties

pytestmark = pytest.mark.gpu

LIST = R.COUNTS + R.TINY40
TYPES = M.cycle(len(LIST))
WIDE = bool(os.environ.get("FTAR_GPU_WIDE"))


@pytest.fixture(scope="module")
def probe():
    return M.build()


def _fn(oracle, algo):
    return oracle.rabenseifner if algo == "raben" else oracle.recursive_doubling


def _cap(vectors, counts, types, what):
    for v in vectors:
        assert M.nan_share(v, counts, types) <= M.NAN_CAP, (what, "too many NaN elements to compare anything")


def _fill(counts, types, per_type):
    """The raw vector of a list whose entries of type t hold, in list order, per_type[t]'s elements."""
    used = {t: 0 for t in per_type}
    out = []
    for c, t in zip(counts, types):
        out.append(per_type[t][used[t]:used[t] + c].view(np.uint8))
        used[t] += c
    assert all(used[t] == per_type[t].size for t in per_type)
    return np.concatenate(out)


F32_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF,
                         0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF],
                        dtype=np.uint32)


def test_every_pattern_round_trips(probe):
    """p = 1, scale 1: no arithmetic, so the output is the input bit for bit (a NaN for a NaN).  The
    float16 entries together hold all 65536 patterns, so do the bfloat16 entries; the float32
    entries hold +-0, +-inf, NaNs, the smallest and largest subnormals and normals and random bit
    patterns.  Types cycle, so neighbours differ; one remainder entry per type ends the list."""
    counts = [1, 3, 0, 5, 255, 256, 257, 4093, 4099, 8193] + R.TINY40
    types = M.cycle(len(counts))
    have = {t: sum(c for c, u in zip(counts, types) if u == t) for t in M.CYCLE}
    for t in M.cycle(3, start=len(counts)):
        counts.append((65536 if t != M.F32 else 30000) - have[t])
        types.append(t)
    assert all(a != b for a, b in zip(types, types[1:])) and min(counts[-3:]) > 0
    rng = np.random.default_rng(5)
    f32 = rng.integers(0, 2 ** 32, size=30000, dtype=np.uint64).astype(np.uint32)
    f32[:F32_SPECIALS.size] = F32_SPECIALS          # entry 0 (one element) of the list is bfloat16: these land in entries 1, 4, ..
    f32[-F32_SPECIALS.size:] = F32_SPECIALS
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x = _fill(counts, types, {M.F16: every, M.BF16: every.copy(), M.F32: f32})
    _cap([x], counts, types, "all patterns")
    for algo, inplace, offset in (("raben", 0, 0), ("raben", 0, 1), ("rd", 1, 0), ("rd", 1, 1)):
        r = M.run_mixed(algo, [(counts, types, [x])], 1, inplace=inplace, offset=offset, timeout=60)
        what = (algo, inplace, offset)
        assert r.returncode == 0, (what, r.stderr[-2000:])
        s = r.status[0][0]
        assert (s[R.RC], s[R.CSIZE]) == (0, 1), (what, s)
        assert s[R.INTACT] == 1, (what, "a guard or an input was written")
        assert s[R.COALESCED] == sum(1 for c in counts if c), (what, s)
        assert s[M.HBM] >= 2 * (4 * sum(counts) + M.nbytes(counts, types)), (what, s)
        assert M.same(r.outputs[0][0], x, counts, types), what


def test_scale_on_the_float32_path(probe):
    """p = 1, scale -0.5 and 2^-20: the float32 entries hold +-0, values whose product is subnormal
    and values whose product no bfloat16 holds; every result is numpy's float32 product bit for
    bit -- -0 kept, nothing passed through 16 bits."""
    rng = np.random.default_rng(9)
    n32 = sum(c for c, t in zip(LIST, TYPES) if t == M.F32)
    n16 = {t: sum(c for c, u in zip(LIST, TYPES) if u == t) for t in (M.F16, M.BF16)}
    for scale in (-0.5, 2.0 ** -20):
        v = (rng.uniform(1, 2, size=n32) * rng.choice([-1, 1], size=n32)).astype(np.float32)
        third = n32 // 3
        v[:third] *= np.float32(2.0 ** -126) if scale == -0.5 else np.float32(2.0 ** -110)  # the product is subnormal
        v[third:third + 8] = np.array([0.0, -0.0] * 4, dtype=np.float32)
        per = {M.F32: v.view(np.uint32)}
        for t in n16:
            per[t] = A.narrow((rng.uniform(-4, 4, size=n16[t])).astype(np.float32), t)
            per[t][:2] = [0x0000, 0x8000]
        x = _fill(LIST, TYPES, per)
        with np.errstate(under="ignore"):
            want = M.narrow_list(np.float32(scale) * M.widen_list(x, LIST, TYPES), LIST, TYPES)
        # the model's float32 entries do what the test is about
        w32 = np.concatenate([want[b:b + 4 * c].view(np.float32) for t, b, e, c in M.pieces(LIST, TYPES) if t == M.F32])
        assert np.array_equal(w32.view(np.uint32), (np.float32(scale) * v).view(np.uint32))
        assert np.any(w32.view(np.uint32) == 0x80000000) and np.any(w32.view(np.uint32) == 0)
        assert np.sum((w32 != 0) & (np.abs(w32) < np.float32(2.0 ** -126))) >= third - 8
        assert np.mean(w32.view(np.uint32) & 0xFFFF != 0) > 0.9
        _cap([want], LIST, TYPES, scale)
        for algo, inplace in (("raben", 0), ("rd", 1)):
            r = M.run_mixed(algo, [(LIST, TYPES, [x])], 1, scale=scale, inplace=inplace, offset=1, timeout=60)
            assert r.returncode == 0, (scale, algo, r.stderr[-2000:])
            s = r.status[0][0]
            assert (s[R.RC], s[R.INTACT], s[R.COALESCED]) == (0, 1, sum(1 for c in LIST if c)), (scale, algo, s)
            got = r.outputs[0][0]
            assert np.array_equal(got, want), (scale, algo, np.flatnonzero(got != want)[:8])  # no NaN in these inputs: plain bit equality


def test_uniform_lists_equal_the_existing_calls(probe, oracle):
    """p = 2, one job: an all-bfloat16 and an all-float16 list with scale 0.5 give
    ftar_allreduce_multi_acc32's output, an all-float32 list with scale 1 gives
    ftar_allreduce_multi(FLOAT32)'s."""
    p = 2
    calls, modes, scales = [], [], []
    for t, scale, other in ((M.BF16, 0.5, 2), (M.F16, 0.5, 2), (M.F32, 1.0, 1)):
        types = [t] * len(LIST)
        ins = M.specials(oracle, p, LIST, types, seed=30 + t)
        calls += [(LIST, types, ins), (LIST, types, ins)]
        modes += [0, other]
        scales += [scale, scale]
    models = [M.model(oracle.rabenseifner, ins, c, t, 0, s) for (c, t, ins), s in zip(calls, scales)]
    for (c, t, _), (_, want) in zip(calls, models):
        _cap(want, c, t, "uniform")
    for algo in ("raben", "rd"):
        r = M.run_mixed(algo, calls, p, op=0, scale=scales, mode=modes, offset=1, timeout=90)
        assert r.returncode == 0, (algo, r.stderr[-2000:])
        for k in range(0, len(calls), 2):
            c, t, ins = calls[k]
            o, want = M.model(_fn(oracle, algo), ins, c, t, 0, scales[k])
            M.check_against_model(o, want, r, k, c, t, (algo, "uniform", k))
            for w in range(p):
                s = r.status[k + 1][w]
                assert (s[R.RC], s[R.INTACT]) == (0, 1), (algo, k, w, s)
                assert M.same(r.outputs[k][w], r.outputs[k + 1][w], c, t), (algo, k, w, "differs from the existing call")


@pytest.mark.parametrize("p", [2, 4, 3, 5])
@pytest.mark.parametrize("algo", ["raben", "rd"])
def test_equals_oracle_and_plain_float32_call(probe, oracle, algo, p):
    """A mixed list, SUM with scale 1 / p and MAX with scale 1, inputs with NaN, +-0 and +-inf.
    Against the model; and the plain float32 entry point, run by the probe in the same job on the
    widened vector, gives after the per-entry scale-and-narrow in numpy the new call's output."""
    fn = _fn(oracle, algo)
    ops, scales = [0, 2], [float(np.float32(1) / np.float32(p)), 1.0]
    calls = [(LIST, TYPES, M.specials(oracle, p, LIST, TYPES, seed=10 * p + seed)) for seed in (1, 2)]
    models = [M.model(fn, ins, c, t, ops[k], scales[k]) for k, (c, t, ins) in enumerate(calls)]
    for _, want in models:
        _cap(want, LIST, TYPES, (algo, p))
    r = M.run_mixed(algo, calls, p, op=ops, scale=scales, plain=True, offset=p % 2, timeout=90)
    assert r.returncode == 0, r.stderr[-2000:]
    for k, (c, t, ins) in enumerate(calls):
        o, want = models[k]
        M.check_against_model(o, want, r, k, c, t, (algo, p, k))
        for w in range(p):
            assert r.status[k][w][R.PLAIN_RC] == 0
            with np.errstate(over="ignore", invalid="ignore", under="ignore"):
                via_plain = M.narrow_list(np.float32(scales[k]) * r.plain[k][w], c, t)
            assert M.same(r.outputs[k][w], via_plain, c, t), (algo, p, k, w, "differs from narrow(scale * plain float32 call)")


def test_ties_beside_a_float32_entry(probe, oracle):
    """p = 2, SUM, scale 1: the 2-byte entries hold acc32's tie construction -- every sum exact in
    float32 and exactly halfway between two patterns, so nearest-even differs from truncation and
    from round-half-away -- and the float32 entry behind each holds the same sums, unrounded."""
    vb, hb = _ties(A.BF16)
    vf, hf = _ties(A.F16)
    counts = [vb.size, vb.size, 3, vf.size, vf.size]
    types = [M.BF16, M.F32, M.F16, M.F16, M.F32]
    three = np.array([0x3C00, 0x4000, 0xBC00], dtype=np.uint16)
    r0 = np.concatenate([a.view(np.uint8) for a in (vb, A.widen(vb, A.BF16), three, vf, A.widen(vf, A.F16))])
    r1 = np.concatenate([a.view(np.uint8) for a in (hb, A.widen(hb, A.BF16), three, hf, A.widen(hf, A.F16))])
    o, want = M.model(oracle.rabenseifner, [r0, r1], counts, types, 0, 1.0)
    _cap(want, counts, types, "ties")
    ent = {i: want[0][b:b + c * M.esize(t)] for i, (t, b, e, c) in enumerate(M.pieces(counts, types))}
    for i, v, dt in ((0, vb, A.BF16), (3, vf, A.F16)):
        t16, s32 = ent[i].view(np.uint16), ent[i + 1].view(np.float32)
        assert np.all((t16 == v) | (t16 == v + 1)) and np.all(t16 & 1 == 0) and 0 < np.sum(t16 == v) < v.size
        fin = np.isfinite(A.widen(t16, dt))
        assert np.all(A.widen(t16, dt)[fin] != s32[fin])  # the float32 neighbour keeps what the rounding dropped
    for algo in ("raben", "rd"):
        r = M.run_mixed(algo, [(counts, types, [r0, r1])], 2, op=0, offset=1, timeout=90)
        assert r.returncode == 0, r.stderr[-2000:]
        o, want = M.model(_fn(oracle, algo), [r0, r1], counts, types, 0, 1.0)
        M.check_against_model(o, want, r, 0, counts, types, (algo, "ties"))


# per schedule one recovering kill and the aborting first-loop-step kill of acc32's KILLS
KILLS = [k for k in ACC32_KILLS if k[2] in ((4, 1, 1, 1), (1, 1, 1, 2), (1, 1, 0, 1))]


@pytest.mark.parametrize("algo,p,kill", KILLS, ids=[f"{a}-p{p}-{'_'.join(map(str, k))}" for a, p, k in KILLS])
def test_kills_end_as_the_oracle_says(probe, oracle, algo, p, kill):
    """A mixed list, SUM: outcome class, return code, comm size, recoveries and the survivors' bits
    are the oracle's on the widened inputs; the aborting case writes no output."""
    counts, types = R.COUNTS, M.cycle(len(R.COUNTS))
    ins = M.specials(oracle, p, counts, types, seed=3 * p)
    o, want = M.model(_fn(oracle, algo), ins, counts, types, 0, 1.0, kills=[kill])
    assert o.aborted == (kill == (1, 1, 0, 1)) and (o.aborted or o.recoveries == 1)
    if not o.aborted:
        _cap([want[w] for w, st in enumerate(o.status) if st == 0], counts, types, kill)
    r = M.run_mixed(algo, [(counts, types, ins)], p, op=0, kills=[kill], timeout=90)
    M.check_against_model(o, want, r, 0, counts, types, (algo, p, kill))


def test_limit_regrowth_and_the_other_movers(probe, oracle):
    """nbufs = FTAR_MULTI_MAX with 1..7 elements each and cycling types, inside a call sequence
    whose totals grow, shrink and grow again, with one ftar_allreduce_multi_acc32 call and one
    ftar_allreduce_multi call in between (the three movers share the staging and the table mirror);
    p = 2, SUM, scale 0.5."""
    p = 2
    lists = [R.TINY40, [1 + (i * 11) % 7 for i in range(1024)], [2, 2], R.COUNTS + [70001, 3], R.COUNTS, R.COUNTS, R.COUNTS]
    modes = [0, 0, 0, 0, 2, 1, 0]
    typs = [M.cycle(len(c)) for c in lists]
    typs[4], typs[5] = [M.BF16] * len(R.COUNTS), [M.F32] * len(R.COUNTS)
    calls = [(c, t, M.specials(oracle, p, c, t, seed=40 + k)) for k, (c, t) in enumerate(zip(lists, typs))]
    scales = [0.5 if m != 1 else 1.0 for m in modes]  # (ftar_allreduce_multi has no scale)
    for algo in ("raben", "rd"):
        models = [M.model(_fn(oracle, algo), ins, c, t, 0, s) for (c, t, ins), s in zip(calls, scales)]
        for (c, t, _), (_, want) in zip(calls, models):
            _cap(want, c, t, "sequence")
        r = M.run_mixed(algo, calls, p, op=0, scale=scales, mode=modes, offset=1, timeout=90)
        assert r.returncode == 0, r.stderr[-2000:]
        for k, (c, t, ins) in enumerate(calls):
            o, want = models[k]
            if modes[k] == 0:
                M.check_against_model(o, want, r, k, c, t, (algo, "sequence", k))
                continue
            for w in range(p):  # the existing calls on their uniform lists: the same definition
                s = r.status[k][w]
                assert (s[R.RC], s[R.INTACT], s[R.COALESCED]) == (0, 1, sum(1 for x in c if x)), (algo, k, w, s)
                assert M.same(r.outputs[k][w], want[w], c, t), (algo, "existing call in between", k, w)


@pytest.mark.parametrize("algo", ["raben", "rd"])
def test_fence_discipline_of_a_mixed_job(probe, oracle, algo):
    """FTAR_TRACE logs of a p = 2 job through tests/fence_check.py's checker, unchanged: a small
    list and, twice, one above the staging limit.  The second large call finds the staging vector
    registered with the trace, so its gather launch shows the packed range it writes: 4 bytes per
    element whatever the entries' types."""
    p = 2
    big = R.COUNTS + [300001, 5]
    lists = [R.COUNTS, big, big]
    calls = [(c, M.cycle(len(c)), M.specials(oracle, p, c, M.cycle(len(c)), seed=90 + k)) for k, c in enumerate(lists)]
    models = [M.model(_fn(oracle, algo), ins, c, t, 0, 0.5) for c, t, ins in calls]
    for (c, t, _), (_, want) in zip(calls, models):
        _cap(want, c, t, "traced")
    tmp = tempfile.mkdtemp(prefix="ftar_mixed_fence_")
    try:
        r = M.run_mixed(algo, calls, p, op=0, scale=0.5, env_extra={"FTAR_TRACE": os.path.join(tmp, "t")}, timeout=90)
        assert r.returncode == 0, r.stderr[-2000:]
        for k, (c, t, ins) in enumerate(calls):
            M.check_against_model(models[k][0], models[k][1], r, k, c, t, (algo, "traced", k))
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
    """Comm.allreduce_multi_mixed on [bf16, f32, f16, empty f32, bf16], p = 2: in place with SUM and
    scale 0.5, then out of place with MAX and algo="rd"."""
    p, counts, types = 2, [4093, 257, 5, 0, 3], [M.BF16, M.F32, M.F16, M.F32, M.BF16]
    jobs = [(oracle.rabenseifner, 0, 0.5), (oracle.recursive_doubling, 2, 1.0)]
    ins = [M.specials(oracle, p, counts, types, seed=77 + k) for k in range(len(jobs))]
    models = [M.model(fn, ins[k], counts, types, op, scale) for k, (fn, op, scale) in enumerate(jobs)]
    for _, want in models:
        _cap(want, counts, types, "torch")
    tmp = tempfile.mkdtemp(prefix="ftar_mixed_torch_")
    try:
        for k, per_rank in enumerate(ins):
            for r, x in enumerate(per_rank):
                x.tofile(os.path.join(tmp, f"in_{r}_{k}.bin"))
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, MULTI_COUNTS=",".join(map(str, counts)), MIXED_TYPES=",".join(map(str, types)))
        env.pop("FTAR_KILL", None)
        cp = subprocess.run([os.path.join(H.PKG, "bin", "ftrun"), "-np", str(p), "--devmap", "0,0", sys.executable, "-u",
                             os.path.join(H.ROOT, "tests", "mixed_worker.py")], env=env, capture_output=True, text=True,
                            timeout=120)
        assert cp.returncode == 0, cp.stderr[-3000:]
        nonempty = sum(1 for c in counts if c)
        for k in range(len(jobs)):
            for w in range(p):
                st = tuple(int(v) for v in open(os.path.join(tmp, f"status_{w}_{k}.txt")).read().split())
                assert st == (0, nonempty, 1), (w, k, st)
                got = np.fromfile(os.path.join(tmp, f"out_{w}_{k}.bin"), dtype=np.uint8)
                assert M.same(got, models[k][1][w], counts, types), (w, k)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_ftbench_mixed():
    """bin/ftbench with FTBENCH_MULTI=7 FTBENCH_MIXED=1 on both schedules, p = 2: its own check
    (every element its exact sum) passes, and hbm_bytes is at least the two movers'."""
    count, multi = 70001, 7
    env = dict(os.environ, FTBENCH_MULTI=str(multi), FTBENCH_MIXED="1", FTBENCH_PATTERN="1")
    env.pop("FTAR_KILL", None)
    env.pop("FTBENCH_ACC32", None)
    per = [count // multi + (k < count % multi) for k in range(multi)]
    movers = 2 * sum(c * (4 + M.esize(M.CYCLE[k % 3])) for k, c in enumerate(per))
    for algo in ("raben", "rd"):
        cp = subprocess.run([os.path.join(H.PKG, "bin", "ftrun"), "-np", "2", "--devmap", "0,0",
                             os.path.join(H.PKG, "bin", "ftbench"), algo, str(count), "2"], env=env, capture_output=True,
                            text=True, timeout=60)
        assert cp.returncode == 0, (algo, cp.stderr[-2000:])
        lines = [json.loads(ln) for ln in cp.stdout.splitlines() if ln.startswith("{")]
        assert sorted(ln["rank"] for ln in lines) == [0, 1]
        for ln in lines:
            assert all(c["rc"] == 0 and c["uniform"] and c["comm_size"] == 2 for c in ln["calls"]), (algo, ln)
            assert all(c["hbm_bytes"] >= movers for c in ln["calls"]), (algo, ln)
