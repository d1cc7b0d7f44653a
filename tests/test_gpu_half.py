"""float16 and bfloat16 on the GPU: the local reduce and both Allreduce schedules, bit for bit.

Every GPU action runs in a child (tests/half_worker.py, directly or as the ranks of an ftrun
job, all on GPU 0 like the other schedule tests): the pytest process never opens the GPU.
Comparisons are on the uint16 bit patterns; where a NaN is expected, on NaN-ness (the payload
of an arithmetic NaN is not specified).

References
* local reduce: the same operation on torch CPU tensors of the element type (one correctly
  rounded operation per element; MAX / MIN as the library's (x > y) ? x : y on (inout, in));
* schedules, order-free inputs: the float32 oracle on the widened inputs, narrowed again --
  exact, because no combination of these inputs rounds in either 16-bit format: MAX / MIN
  select (with NaN, signed zeros and infinities placed to pin the operand order), SUM of
  integers in [-8, 8] (|partial sums| <= 8 * 16 = 128 < 2^8, the bfloat16 significand), PROD of
  +-0.5, +-1, +-2 (powers of two, 2^-9 .. 2^9 at p <= 9: normal in both formats);
* schedules, rounding: half_model.py's trees (validated against the oracle in
  test_half_abi.py) with a torch CPU addition in the element type at every node.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import half_model as M
import harness as H

pytestmark = pytest.mark.gpu

ALL_ON_GPU0 = ",".join(["0"] * 16)
WORKER = os.path.join(H.ROOT, "tests", "half_worker.py")
TD = {"f16": torch.float16, "bf16": torch.bfloat16}
SUM, PROD, MAX, MIN = 0, 1, 2, 3


# ---- bit patterns <-> values (torch CPU) -----------------------------------------------
def tens(u16, name):
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16).copy()).view(TD[name])


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def to_bits(f32, name):
    return bits(torch.from_numpy(np.ascontiguousarray(f32, dtype=np.float32)).to(TD[name]))


def to_f32(u16, name):
    return tens(u16, name).float().numpy()


def pair(name, op):
    """inout <op> in on uint16 bit patterns: one torch CPU operation in the element type."""
    def f(x, y):
        a, b = tens(x, name), tens(y, name)
        if op == SUM:
            r = a + b
        elif op == PROD:
            r = a * b
        elif op == MAX:
            r = torch.where(a > b, a, b)
        else:
            r = torch.where(a < b, a, b)
        return bits(r)
    return f


def assert_same_bits(got, want, name, what):
    """Bit equality, NaN-ness where the reference holds a NaN."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_w, nan_g = np.isnan(to_f32(want, name)), np.isnan(to_f32(got, name))
    assert np.array_equal(nan_w, nan_g), (what, "NaN places", np.flatnonzero(nan_w != nan_g)[:8])
    bad = np.flatnonzero((got != want) & ~nan_w)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def finite_random_bits(rng, n, name):
    """Random bit patterns, the non-finite ones (exponent all ones) replaced by finite ones."""
    x = rng.integers(0, 1 << 16, size=n, dtype=np.uint16)
    emask = 0x7C00 if name == "f16" else 0x7F80
    x[(x & emask) == emask] &= np.uint16(0xBFFF)  # clear the exponent's top bit: finite
    return x


def specials(name, op):
    """Pairs (inout, in): signed zeros, infinities, the largest and smallest normal, subnormals,
    sums and products that overflow, underflow and cancel; NaN for SUM / PROD only."""
    fi = torch.finfo(TD[name])
    big, tiny, sub = fi.max, fi.tiny, fi.smallest_normal * fi.eps  # sub: the smallest subnormal
    inf, nan = float("inf"), float("nan")
    ps = [(0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, 0.0), (inf, -inf), (-inf, inf), (inf, 1.0), (1.0, -inf),
          (big, big), (-big, -big), (big, -big), (big, 2.0), (big, fi.eps * big), (big, 1.0), (tiny, tiny),
          (tiny, -tiny), (tiny, 0.5), (tiny, sub), (sub, sub), (sub, -sub), (sub, 0.5), (-sub, 0.5), (3 * sub, 0.5),
          (tiny - sub, sub), (tiny - sub, 1.0), (1.0, fi.eps / 2), (1.0 + fi.eps, fi.eps / 2), (big, inf), (0.0, inf),
          (-0.0, sub), (1.0, -1.0), (inf, 0.0)]
    if op in (SUM, PROD):
        ps += [(nan, 1.0), (1.0, nan), (nan, nan), (nan, inf), (-inf, nan)]
    a = torch.tensor([p[0] for p in ps], dtype=torch.float64).to(TD[name])
    b = torch.tensor([p[1] for p in ps], dtype=torch.float64).to(TD[name])
    return bits(a), bits(b)


# ---- children ------------------------------------------------------------------------
def run_child(cmd, env, timeout):
    """One child under a timeout; the test stops at the first one that fails."""
    cp = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    return cp


def run_job(name, algo_calls, inputs, p, env_extra=None, kills=(), timeout=120):
    """An ftrun job of p half_worker ranks.  algo_calls: the worker's call list; inputs[k][r]:
    rank r's uint16 vector of call k.  Returns (completed process, out[k][r], status[k][r])."""
    tmp = tempfile.mkdtemp(prefix="ftar_half_")
    try:
        json.dump(algo_calls, open(os.path.join(tmp, "calls.json"), "w"))
        for k, per_rank in enumerate(inputs):
            for r, x in enumerate(per_rank):
                np.ascontiguousarray(x, dtype=np.uint16).tofile(os.path.join(tmp, f"in_{r}_{k}.bin"))
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, HALF_MODE="sched", HALF_DTYPE=name)
        env.pop("FTAR_KILL", None)
        if kills:
            env["FTAR_KILL"] = H.kill_env(kills)
        env.update(env_extra or {})
        cp = run_child([os.path.join(H.PKG, "bin", "ftrun"), "-np", str(p), "--devmap", ALL_ON_GPU0, sys.executable,
                        "-u", WORKER], env, timeout)
        outs, stats = [], []
        for k in range(len(algo_calls)):
            o, s = {}, {}
            for r in range(p):
                f, g = os.path.join(tmp, f"out_{r}_{k}.bin"), os.path.join(tmp, f"status_{r}_{k}.txt")
                if os.path.exists(f) and os.path.exists(g):
                    o[r] = np.fromfile(f, dtype=np.uint16)
                    s[r] = tuple(int(v) for v in open(g).read().split())
            outs.append(o)
            stats.append(s)
        return cp, outs, stats
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def call(algo, op, inplace=0, offset=0, host=0):
    return {"algo": algo, "op": op, "inplace": inplace, "offset": offset, "host": host}


# ---- inputs of the schedule tests ------------------------------------------------------
def order_free_inputs(name, op, p, count, seed):
    """Per-rank uint16 vectors whose reduction rounds nowhere (module docstring)."""
    rng = np.random.default_rng(seed)
    if op in (MAX, MIN):
        f = [to_f32(to_bits((rng.random(count) * 2 - 1).astype(np.float32), name), name) for _ in range(p)]
        f = H.with_specials(f, seed + 1)
    elif op == SUM:
        f = [rng.integers(-8, 9, size=count).astype(np.float32) for _ in range(p)]
    else:
        f = [rng.choice(np.array([-2, -1, -0.5, 0.5, 1, 2], dtype=np.float32), size=count) for _ in range(p)]
    return [to_bits(x, name) for x in f]


def check_against_oracle(oracle, name, algo, op, ins, kills, outs, stats, cp, what):
    fn = oracle.rabenseifner if algo == "raben" else oracle.recursive_doubling
    o = fn([to_f32(x, name) for x in ins], kills, op=op)
    if o.aborted:  # the outcome class is the oracle's: MPI_Abort, no rank returns
        assert "MPI_ABORT" in cp.stderr and not outs, (what, cp.stderr[-2000:])
        return
    assert "MPI_ABORT" not in cp.stderr, (what, cp.stderr[-2000:])
    for w, st in enumerate(o.status):
        if st != 0:
            assert w not in outs, (what, "rank", w, "died in the oracle")
            continue
        assert w in outs, (what, "rank", w, cp.stderr[-2000:])
        rc, size_after, recoveries, intact = stats[w]
        assert (rc, size_after, recoveries) == (o.ret, len(o.order_after), o.recoveries), (what, w, stats[w])
        assert intact == 1, (what, w, "guards or send buffer written")
        assert_same_bits(outs[w], to_bits(o.outputs[w], name), name, (what, "rank", w))


def rounding_inputs(name, p, count, seed):
    rng = np.random.default_rng(seed)
    return [finite_random_bits(rng, count, name) for _ in range(p)]


def check_rounding(name, algo, ins, outs, stats, what):
    """SUM of random finite values: the schedule's tree with a 16-bit addition at every node."""
    p = len(ins)
    want = M.raben_tree(ins, pair(name, SUM)) if algo == "raben" else M.rd_tree(ins, pair(name, SUM))[0]
    if p == 2:  # one addition
        assert_same_bits(want, pair(name, SUM)(ins[0], ins[1]), name, (what, "model at p = 2"))
    for w in range(p):
        assert stats[w][0] == 0 and stats[w][3] == 1, (what, w, stats[w])
        assert np.array_equal(outs[w], outs[0]), (what, "ranks", w, "and 0 differ")  # bit for bit, NaN included
        assert_same_bits(outs[w], want, name, (what, "rank", w))


# ---- 1. local reduce -------------------------------------------------------------------
LOCAL_N = [0, 1, 7, 8, 9, 15, 17, 1031, 16397]
LOCAL_OFFSETS = [(1, 1), (3, 3), (7, 7), (2, 6), (1, 2), (0, 5)]
N_LDS = 3 * 8192 + 40


def _local_cases():
    cases = []
    for name in ("f16", "bf16"):
        for op in (SUM, PROD, MAX, MIN):
            cases += [dict(dtype=name, op=op, n=n, off_in=0, off_io=0, variant=1) for n in LOCAL_N]
            cases += [dict(dtype=name, op=op, n=16397, off_in=a, off_io=b, variant=1) for a, b in LOCAL_OFFSETS]
            cases += [dict(dtype=name, op=op, n=N_LDS, off_in=0, off_io=0, variant=v) for v in (0, 1)]
    return cases


def test_local_reduce_matrix():
    """ftar_reduce_local, both types x SUM / PROD / MAX / MIN: sizes around the 8-element vector
    and the 8192-element tile, unaligned windows (co-aligned: heads of 7, 5 and 1 elements; not
    co-aligned: the scalar path) with everything outside the window untouched, and both
    local-reduce kernels.  One child runs the whole matrix."""
    cases = _local_cases()
    rng = np.random.default_rng(16)
    tmp = tempfile.mkdtemp(prefix="ftar_half_local_")
    try:
        bufs = []
        for i, c in enumerate(cases):
            n, name = c["n"], c["dtype"]
            a = finite_random_bits(rng, n + c["off_in"] + 16, name)
            b = finite_random_bits(rng, n + c["off_io"] + 16, name)
            sb, sa = specials(name, c["op"])  # (inout, in)
            m = min(n, sa.size)
            a[c["off_in"]:c["off_in"] + m] = sa[:m]
            b[c["off_io"]:c["off_io"] + m] = sb[:m]
            a.tofile(os.path.join(tmp, f"lin_{i}.bin"))
            b.tofile(os.path.join(tmp, f"lio_{i}.bin"))
            bufs.append((a, b))
        json.dump(cases, open(os.path.join(tmp, "cases.json"), "w"))
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, HALF_MODE="local", HALF_DTYPE="bf16")
        cp = run_child([sys.executable, "-u", WORKER], env, 120)
        assert cp.returncode == 0, cp.stderr[-3000:]
        status = [tuple(int(v) for v in ln.split()) for ln in open(os.path.join(tmp, "status.txt"))]
        assert len(status) == len(cases)
        for i, c in enumerate(cases):
            a, b = bufs[i]
            n, oi, ob, name = c["n"], c["off_in"], c["off_io"], c["dtype"]
            got = np.fromfile(os.path.join(tmp, f"lout_{i}.bin"), dtype=np.uint16)
            assert status[i] == (0, 1), (c, status[i])
            want = b.copy()
            want[ob:ob + n] = pair(name, c["op"])(b[ob:ob + n], a[oi:oi + n])
            assert np.array_equal(got[:ob], b[:ob]) and np.array_equal(got[ob + n:], b[ob + n:]), (c, "outside the window")
            assert_same_bits(got[ob:ob + n], want[ob:ob + n], name, c)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---- 2. schedules against the oracle ---------------------------------------------------
BOTH, BF = ("f16", "bf16"), ("bf16",)
TREE = {"FTAR_ONESHOT_MAX": "0"}
# (id, algo, p, count, settings, kill, element types): both types where the form is new ground
# for 2-byte elements (one-shot, tree, step by step, push), bfloat16 alone elsewhere
MATRIX = [
    ("oneshot_p8", "raben", 8, 4099, {}, None, BOTH),
    ("tree_p4", "raben", 4, 65541, TREE, None, BOTH),
    ("tree_u4_p4", "raben", 4, 65541, dict(TREE, FTAR_TREE_UNROLL="4"), None, BF),
    ("steps_p4", "raben", 4, 65541, {"FTAR_MESH": "0"}, None, BOTH),
    ("push_p4", "raben", 4, 65541, {"FTAR_PUSH": "2"}, None, BOTH),
    ("copy_engine_p4", "raben", 4, 65541, {"FTAR_COPY_ENGINE": "1", "FTAR_RELAY": "0", "FTAR_MESH": "0"}, None, BF),
    ("heads_p2", "raben", 2, 7, {}, None, BF),
    ("prepost_p5", "raben", 5, 1031, {}, None, BF),
    # a death in reduce-scatter step 0 is fatal in the reference (raben/errhandler.c:37-38): the
    # oracle aborts and so must the job; the same victim point one step later recovers
    ("kill_step0_p5", "raben", 5, 1031, {}, (1, 1, 0, 1), BF),
    ("recovery_p5", "raben", 5, 1031, {}, (4, 1, 1, 1), BF),
    ("midexchange_p9", "raben", 9, 65541, {}, (5, 1, 1, 3), BF),
    ("rd_gated_p4", "rd", 4, 1031, {}, None, BF),
    ("rd_large_p4", "rd", 4, (1 << 19) + 3, {}, None, BF),
    ("rd_recovery_p6", "rd", 6, 1031, {}, (3, 1, 1, 3), BF),
]
# the rounding case that rides along as one more call of a job with the same algo, p and settings
ROUNDING_IN = {"oneshot_p8", "steps_p4", "rd_gated_p4", "heads_p2"}
CASES = [pytest.param(*row[:6], name, id=f"{row[0]}-{name}") for row in MATRIX for name in row[6]]


@pytest.mark.parametrize("cid,algo,p,count,settings,kill,name", CASES)
def test_schedule_against_oracle(oracle, cid, algo, p, count, settings, kill, name):
    """MAX, MIN, SUM and PROD of order-free inputs through one form of a schedule.  Without a
    kill the four are four calls of one job (plus, where ROUNDING_IN says so, the rounding SUM of
    section 3 in the same form); a kill case is one job per op, and its return code, comm size
    after the call and recoveries are the oracle's too."""
    ops = (MAX, MIN, SUM, PROD)
    ins = {op: order_free_inputs(name, op, p, count, seed=1000 + 10 * p + op) for op in ops}
    if kill:
        fn = oracle.rabenseifner if algo == "raben" else oracle.recursive_doubling
        o = fn([to_f32(x, name) for x in ins[SUM]], [kill], op=SUM)
        assert o.aborted == (cid == "kill_step0_p5") and (o.aborted or o.recoveries == 1), (cid, o.aborted, o.recoveries)
        for op in ops:
            cp, outs, stats = run_job(name, [call(algo, op)], [ins[op]], p, settings, [kill])
            check_against_oracle(oracle, name, algo, op, ins[op], [kill], outs[0], stats[0], cp, (cid, name, op))
        return
    calls = [call(algo, op) for op in ops]
    data = [ins[op] for op in ops]
    if cid in ROUNDING_IN:
        calls.append(call(algo, SUM))
        data.append(rounding_inputs(name, p, count, seed=p + count))
    cp, outs, stats = run_job(name, calls, data, p, settings)
    assert cp.returncode == 0, cp.stderr[-3000:]
    for k, op in enumerate(ops):
        check_against_oracle(oracle, name, algo, op, ins[op], [], outs[k], stats[k], cp, (cid, name, op))
    if cid in ROUNDING_IN:
        check_rounding(name, algo, data[4], outs[4], stats[4], (cid, name, "rounding"))


def test_inplace_offset_and_host_buffers(oracle):
    """sbuf == rbuf, windows at element offset 3 (6 bytes: a 5-element head, then vectors), and
    the *_host entry points on pageable buffers (H2D, device Allreduce, D2H), bfloat16: the
    tree form at p = 4 in one job, both host entry points at p = 2 in another."""
    name = "bf16"
    calls = [call("raben", MAX, inplace=1), call("raben", SUM, offset=3), call("rd", MIN, inplace=1, offset=3)]
    data = [order_free_inputs(name, c["op"], 4, 65541, seed=40 + k) for k, c in enumerate(calls)]
    cp, outs, stats = run_job(name, calls, data, 4, TREE)
    assert cp.returncode == 0, cp.stderr[-3000:]
    for k, c in enumerate(calls):
        check_against_oracle(oracle, name, c["algo"], c["op"], data[k], [], outs[k], stats[k], cp, ("device", k))
    calls = [call("raben", MAX, host=1), call("rd", MAX, host=1), call("raben", SUM, host=1, offset=3),
             call("rd", PROD, host=1, offset=3)]
    data = [order_free_inputs(name, c["op"], 2, 4099, seed=50 + k) for k, c in enumerate(calls)]
    cp, outs, stats = run_job(name, calls, data, 2)
    assert cp.returncode == 0, cp.stderr[-3000:]
    for k, c in enumerate(calls):
        check_against_oracle(oracle, name, c["algo"], c["op"], data[k], [], outs[k], stats[k], cp, ("host", k))


# ---- 3. schedules, rounding ------------------------------------------------------------
# raben default at p = 8 and p = 2, raben FTAR_MESH=0 at p = 4 and rd at p = 4 ride in section 2's
# jobs (ROUNDING_IN); the rest of {raben, raben FTAR_MESH=0, rd} x {2, 4, 8} is here
ROUNDING = [("raben", 2, 1031, {}), ("rd", 2, 1031, {}), ("raben", 4, 4099, {}), ("raben", 8, 4099, {"FTAR_MESH": "0"}),
            ("rd", 8, 4099, {})]


@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_schedule_rounding(name):
    """SUM of random finite values rounds at every node of the schedule's tree: one torch CPU
    addition at p = 2, the validated tree model with a 16-bit pairwise addition at p = 4 and 8;
    all ranks agree bit for bit.  float16 sums overflow to infinity here and there, and
    inf + -inf gives NaN further up the tree: compared as such."""
    for algo, p, count, settings in ROUNDING:
        ins = rounding_inputs(name, p, count, seed=7 * p + count)
        cp, outs, stats = run_job(name, [call(algo, SUM)], [ins], p, settings)
        assert cp.returncode == 0, (algo, p, cp.stderr[-3000:])
        assert sorted(outs[0]) == list(range(p)), (algo, p, cp.stderr[-2000:])
        check_rounding(name, algo, ins, outs[0], stats[0], (algo, p, settings))
