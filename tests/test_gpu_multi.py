"""ftar_allreduce_multi on the GPU: the table-driven gather / scatter kernel and the call's
contract -- exactly the plain schedule on the dense concatenation of the entries, bit for bit.

Every GPU action runs in a child: tests/multi/multi_probe.c (built against libftar.so, every
entry in a hipMalloc'd buffer of its own with guards on both sides) or tests/multi_worker.py
(the torch binding) as the ranks of an ftrun job, all on GPU 0.  The pytest process never opens
the GPU; every child has its own timeout and a test stops at the first child that fails.

* p = 1: no exchange, so the result is a copy and what is checked is the two kernels alone --
  sizes around a vector and a 16 KiB tile, 40 tiny entries inside one tile, element sizes 2, 4, 8
  and 16 bytes, buffers 0 and 1 elements past a 16-byte boundary (co-aligned with their packed
  offset or not, entry by entry), guards, inputs, in place;
* p = 2, 4 (one-shot / mesh) and 3, 5 (pre-step): both schedules against the unchanged oracle
  on np.concatenate(inputs) and against the plain entry point on one buffer in the same job;
* kills, the 1024-entry limit, staging regrowth, the torch binding, and the fence checker on
  the FTAR_TRACE logs of a multi job.
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fence_check as FC
import harness as H
import multi_runner as R

pytestmark = pytest.mark.gpu

# sizes around a vector and a tile, more than one tile, an empty entry, 40 tiny ones
P1_COUNTS = [1, 3, 0, 5, 4093, 4099, 8193, 2, 2] + R.TINY40
if sum(P1_COUNTS) % 2 == 0:
    P1_COUNTS = P1_COUNTS + [1]  # an odd total: at 2 bytes the vector ends inside a 4-byte word
# (ftar_dtype, op, element bytes)
P1_TYPES = {"float32": (1, 0, 4), "bfloat16": (17, 0, 2), "int64": (2, 0, 8), "double_int_maxloc": (34, 16, 16)}


@pytest.fixture(scope="module")
def probe():
    return R.build(gpu=True)


@pytest.mark.parametrize("name", list(P1_TYPES))
def test_one_rank_is_a_copy(probe, name):
    """The kernels alone.  Four jobs of one rank: buffers 0 and 1 elements past a 16-byte
    boundary, out of place through Rabenseifner's entry and in place through recursive doubling's
    (the single-rank path behind them is shared); each job also runs the plain entry point on
    the dense vector (an odd total: at 2 bytes the copy that dropped the last element)."""
    dt, op, es = P1_TYPES[name]
    rng = np.random.default_rng(es)
    x = rng.integers(0, 256, size=sum(P1_COUNTS) * es, dtype=np.uint8)
    for algo, inplace, offset in (("raben", 0, 0), ("raben", 0, 1), ("rd", 1, 0), ("rd", 1, 1)):
        r = R.run_multi(algo, [(P1_COUNTS, [x])], 1, dtype=dt, op=op, backend="gpu", inplace=inplace, offset=offset,
                        plain=True, timeout=60)
        what = (name, algo, inplace, offset)
        assert r.returncode == 0, (what, r.stderr[-2000:])
        s = r.status[0][0]
        assert (s[R.RC], s[R.CSIZE], s[R.PLAIN_RC]) == (0, 1, 0), (what, s)
        assert s[R.INTACT] == 1, (what, "a guard or an input was written")
        assert s[R.COALESCED] == sum(1 for c in P1_COUNTS if c), (what, s)
        assert R.same_bits(r.outputs[0][0], x), what
        assert R.same_bits(r.plain[0][0], x), (what, "the plain entry point")


def test_plain_single_rank_copy_keeps_the_last_2_byte_element(probe):
    """The plain entry points at comm size 1, out of place, a 2-byte type with an odd count: the
    copy moved bytes / 4 int32 elements and dropped the last element (ftar_single_rank)."""
    x = np.random.default_rng(2).integers(0, 256, size=2 * 1031, dtype=np.uint8)
    for algo in ("raben", "rd"):
        # one non-empty entry: straight through to the plain entry point; and the plain call itself
        r = R.run_multi(algo, [([0, 1031, 0], [x])], 1, dtype=16, op=0, backend="gpu", plain=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.status[0][0][R.RC] == 0 and r.status[0][0][R.PLAIN_RC] == 0 and r.status[0][0][R.COALESCED] == 0
        assert R.same_bits(r.plain[0][0], x), (algo, "plain", r.plain[0][0][-4:], x[-4:])
        assert R.same_bits(r.outputs[0][0], x), (algo, "straight through")


def _three_calls(oracle, p, counts, seed):
    """int32 SUM, float32 SUM and float32 MAX with specials: (calls, dtypes, ops)."""
    n = sum(counts)
    i32 = oracle.random_inputs(p, n, seed=seed, dtype=np.int32)
    f32 = H.with_specials(oracle.random_inputs(p, n, seed=seed + 1, dtype=np.float32), seed)
    g32 = H.with_specials(oracle.random_inputs(p, n, seed=seed + 2, dtype=np.float32), seed + 1)
    return [(counts, i32), (counts, f32), (counts, g32)], [0, 1, 1], [0, 0, 2]


@pytest.mark.parametrize("p", [2, 4, 3, 5])
@pytest.mark.parametrize("algo", ["raben", "rd"])
def test_equals_oracle_and_plain_call(probe, oracle, algo, p):
    """Three calls of one job, every buffer one element past a 16-byte boundary: int32 SUM, float32
    SUM and float32 MAX, both float inputs with NaN, signed zeros and infinities.  Against the
    plain entry point on one buffer in the same job every comparison is bit for bit, NaN payloads
    included.  Against the oracle too, with one exception the header's contract makes: where the
    float SUM yields a NaN its payload is unspecified.  Measured on an MI355X with these inputs:
    recursive doubling at p = 4 differs from the CPU oracle in 1 of 8367 elements, at p = 5 in 5,
    the plain entry point in exactly the same ones (multi != plain: 0 elements); each is a NaN in
    both, 0x7fc00000 against 0xffc00000 -- inf + -inf has the sign bit set on the oracle's x86 and
    clear on the GPU.  So for the SUM call an element may differ from the oracle only where both
    hold a NaN, and only in exactly the elements in which the plain entry point's result of the
    same job differs from the oracle as well; everything else is bit for bit."""
    fn = oracle.rabenseifner if algo == "raben" else oracle.recursive_doubling
    counts = R.COUNTS + R.TINY40
    calls, dts, ops = _three_calls(oracle, p, counts, seed=10 * p)
    r = R.run_multi(algo, calls, p, dtype=dts, op=ops, backend="gpu", plain=True, offset=1, timeout=90)
    assert r.returncode == 0, r.stderr[-2000:]
    for k, (c, ins) in enumerate(calls):
        R.check_against_oracle(fn(ins, op=ops[k]), r, k, c, (algo, p, k), nan_payload=not (dts[k] == 1 and ops[k] == 0))
        want = fn(ins, op=ops[k]).outputs
        for w in range(p):
            assert r.status[k][w][R.PLAIN_RC] == 0
            assert R.same_bits(r.outputs[k][w], r.plain[k][w]), (algo, p, k, w, "multi and plain differ")
            if dts[k] == 1 and ops[k] == 0:  # the elements that differ from the oracle: the plain call's, NaN in both
                u = np.uint32
                bad = np.flatnonzero(r.outputs[k][w].view(u) != want[w].view(u))
                assert np.array_equal(bad, np.flatnonzero(r.plain[k][w].view(u) != want[w].view(u))), (algo, p, k, w)
                assert np.all(np.isnan(r.outputs[k][w][bad])) and np.all(np.isnan(want[w][bad])), (algo, p, k, w)


# per schedule the kills the existing suites use (the oracle: both recover) and one that dies in
# the first loop step, which the reference cannot recover from (the oracle: MPI_Abort)
KILLS = [("raben", 5, (4, 1, 1, 1)), ("raben", 5, (3, 2, 0, 1)), ("raben", 5, (1, 1, 0, 1)),
         ("rd", 6, (1, 1, 1, 2)), ("rd", 6, (3, 1, 1, 3)), ("rd", 6, (1, 1, 0, 1))]


@pytest.mark.parametrize("algo,p,kill", KILLS, ids=[f"{a}-p{p}-{'_'.join(map(str, k))}" for a, p, k in KILLS])
def test_kills_end_as_the_oracle_says(probe, oracle, algo, p, kill):
    fn = oracle.rabenseifner if algo == "raben" else oracle.recursive_doubling
    ins = H.with_specials(oracle.random_inputs(p, sum(R.COUNTS), seed=3 * p, dtype=np.float32), p)
    o = fn(ins, [kill], op=2)
    assert o.aborted == (kill == (1, 1, 0, 1)) and (o.aborted or o.recoveries == 1)
    r = R.run_multi(algo, [(R.COUNTS, ins)], p, dtype=1, op=2, kills=[kill], backend="gpu", timeout=90)
    R.check_against_oracle(o, r, 0, R.COUNTS, (algo, p, kill))


def test_limit_and_staging_regrowth(probe, oracle):
    """nbufs = FTAR_MULTI_MAX with 1..7 elements each, inside a call sequence whose totals grow,
    shrink and grow again (the staging and the kernel's table regrow), p = 2, float32 MAX."""
    p = 2
    lists = [R.TINY40, [1 + (i * 11) % 7 for i in range(1024)], [2, 2], R.COUNTS + [70001, 3], R.COUNTS]
    calls = [(c, H.with_specials(oracle.random_inputs(p, sum(c), seed=40 + k, dtype=np.float32), k)) for k, c in enumerate(lists)]
    for algo in ("raben", "rd"):
        fn = oracle.rabenseifner if algo == "raben" else oracle.recursive_doubling
        r = R.run_multi(algo, calls, p, dtype=1, op=2, backend="gpu", timeout=90)
        assert r.returncode == 0, r.stderr[-2000:]
        for k, (c, ins) in enumerate(calls):
            R.check_against_oracle(fn(ins, op=2), r, k, c, (algo, "sequence", k))


def test_torch_binding(oracle):
    """Comm.allreduce_multi on lists of torch tensors, p = 2: in place with the default schedule,
    out of place with algo="rd" and MAX, and packed FLOAT_INT pairs with MAXLOC."""
    p, counts = 2, [1, 3, 0, 5, 4093, 2]
    ins = oracle.random_inputs(p, sum(counts), seed=77, dtype=np.float32)
    tmp = tempfile.mkdtemp(prefix="ftar_multi_torch_")
    try:
        for r, x in enumerate(ins):
            x.tofile(os.path.join(tmp, f"in_{r}.bin"))
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, MULTI_COUNTS=",".join(map(str, counts)))
        env.pop("FTAR_KILL", None)
        cp = subprocess.run([os.path.join(H.PKG, "bin", "ftrun"), "-np", str(p), "--devmap", "0,0", sys.executable, "-u",
                             os.path.join(H.ROOT, "tests", "multi_worker.py")], env=env, capture_output=True, text=True,
                            timeout=120)
        assert cp.returncode == 0, cp.stderr[-3000:]
        want = [oracle.rabenseifner(ins).outputs, oracle.recursive_doubling(ins, op=2).outputs]
        nonempty = sum(1 for c in counts if c)
        for w in range(p):
            for k in (0, 1):
                st = tuple(int(v) for v in open(os.path.join(tmp, f"status_{w}_{k}.txt")).read().split())
                assert st == (0, nonempty, 1), (w, k, st)
                got = np.fromfile(os.path.join(tmp, f"out_{w}_{k}.bin"), dtype=np.float32)
                assert R.same_bits(got, want[k][w]), (w, k)
            st = tuple(int(v) for v in open(os.path.join(tmp, f"status_{w}_2.txt")).read().split())
            assert st == (0, nonempty, 1), (w, st)
            got = np.fromfile(os.path.join(tmp, f"out_{w}_2.bin"), dtype=np.uint8).view(np.dtype([("v", "<f4"), ("i", "<i4")]))
            # MAXLOC: the larger value, at equal values the lower index (rank 0's); no NaN here
            win = np.where(ins[1] > ins[0], 1, 0)
            assert np.array_equal(got["v"].view(np.uint32), np.where(win == 1, ins[1], ins[0]).view(np.uint32)), w
            assert np.array_equal(got["i"], np.arange(sum(counts)) + win * sum(counts)), w
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.mark.parametrize("algo", ["raben", "rd"])
def test_fence_discipline_of_a_multi_job(probe, oracle, algo):
    """FTAR_TRACE logs of a p = 2 job through tests/fence_check.py's checker, unchanged: a small
    list (staged input, gated launches) and one above the staging limit, whose gathered vector
    the peer reads in place -- the gather's stores must be released before the first barrier."""
    p = 2
    lists = [R.COUNTS, R.COUNTS + [300001]]
    calls = [(c, oracle.random_inputs(p, sum(c), seed=90 + k, dtype=np.float32)) for k, c in enumerate(lists)]
    tmp = tempfile.mkdtemp(prefix="ftar_multi_fence_")
    try:
        r = R.run_multi(algo, calls, p, dtype=1, op=0, backend="gpu", env_extra={"FTAR_TRACE": os.path.join(tmp, "t")},
                        timeout=90)
        assert r.returncode == 0, r.stderr[-2000:]
        fn = oracle.rabenseifner if algo == "raben" else oracle.recursive_doubling
        for k, (c, ins) in enumerate(calls):
            R.check_against_oracle(fn(ins), r, k, c, (algo, "traced", k))
        logs = FC.load(os.path.join(tmp, "t"))
        assert sorted(logs) == list(range(p))
        rep = FC.check(logs)
        assert rep.ok, (rep.release[:5], rep.acquire[:5])
        assert rep.reads_checked > 0
        # the gather and scatter launches are in the log with the packed regions they touch
        text = open(os.path.join(tmp, "t.0")).read()
        assert sum(1 for ln in text.splitlines() if ln.startswith("L ") and " eng=k " in ln) >= 4
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_ftbench_multi():
    """bin/ftbench with FTBENCH_MULTI=7: the job's count split into 7 separately allocated buffers
    and reduced with ftar_allreduce_multi; its own check (every element its exact sum) and its
    output line are the plain job's."""
    import json
    env = dict(os.environ, FTBENCH_MULTI="7", FTBENCH_PATTERN="1")
    env.pop("FTAR_KILL", None)
    for algo in ("raben", "rd"):
        cp = subprocess.run([os.path.join(H.PKG, "bin", "ftrun"), "-np", "2", "--devmap", "0,0",
                             os.path.join(H.PKG, "bin", "ftbench"), algo, "70001", "2"], env=env, capture_output=True,
                            text=True, timeout=60)
        assert cp.returncode == 0, cp.stderr[-2000:]
        lines = [json.loads(ln) for ln in cp.stdout.splitlines() if ln.startswith("{")]
        assert sorted(ln["rank"] for ln in lines) == [0, 1]
        for ln in lines:
            assert all(c["rc"] == 0 and c["uniform"] and c["comm_size"] == 2 for c in ln["calls"]), ln
