"""MAXLOC / MINLOC on MPI's pair types on the GPU: the local reduce and both Allreduce schedules,
byte for byte.

Every GPU action runs in a child (tests/pair_worker.py, directly or as the ranks of an ftrun
job, all on GPU 0 like the other schedule tests): the pytest process never opens the GPU.
Buffers travel as raw bytes and are compared as raw bytes: the result of a pair op is one of
its operands copied whole, the padding of FTAR_DOUBLE_INT included.

References
* local reduce, and the trees of section 3: include/ftar.h's rule written directly in numpy on
  structured arrays (loc): x if x.v > y.v (MINLOC: <) or (x.v == y.v and x.i < y.i), else y;
* schedules with kills: the unchanged oracle.  Values are integers in [-8, 8] and indices
  rank * count + i (distinct, in [0, 2^31)), so MAXLOC is the int64 MAX of the keys
  v * 2^32 + (2^31 - 1 - index) and MINLOC the int64 MIN of v * 2^32 + index: the oracle runs
  those with the same kills, and its result key decodes to the pair every survivor must hold.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import half_model as M
import harness as H

pytestmark = pytest.mark.gpu

ALL_ON_GPU0 = ",".join(["0"] * 16)
WORKER = os.path.join(H.ROOT, "tests", "pair_worker.py")
MAXLOC, MINLOC = 16, 17
OPS = (MAXLOC, MINLOC)
ORACLE_MAX, ORACLE_MIN = 2, 3
ST = {"float_int": np.dtype([("v", "<f4"), ("i", "<i4")]),
      "2int": np.dtype([("v", "<i4"), ("i", "<i4")]),
      "double_int": np.dtype([("v", "<f8"), ("i", "<i4"), ("pad", "<u4")])}
assert [ST[k].itemsize for k in ("float_int", "2int", "double_int")] == [8, 8, 16]
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def loc(op):
    """inout <op> in on structured arrays (x = inout, y = in): the header's rule, whole elements."""
    def f(x, y):
        with np.errstate(invalid="ignore"):
            t = (x["v"] > y["v"]) if op == MAXLOC else (x["v"] < y["v"])
            t = t | ((x["v"] == y["v"]) & (x["i"] < y["i"]))
        out = np.array(y, copy=True)
        out[t] = x[t]
        return out
    return f


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    g, w = raw(got).reshape(got.size, got.itemsize), raw(want).reshape(want.size, want.itemsize)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def fill_padding(a, rng):
    if "pad" in a.dtype.names:
        a["pad"] = rng.integers(0, 1 << 32, size=a.size, dtype=np.uint32)
    return a


def special_pairs(name):
    """(inout, in) pairs as (x.v, x.i, y.v, y.i): ties to the lower index on either side, equal
    value and index (y's bytes, which differ in the +-0 bits or the padding), signed zeros,
    infinities, NaN on either or both sides, the int32 extremes, negative indices."""
    inf, nan = float("inf"), float("nan")
    ps = [(1, 2, 1, 5), (1, 5, 1, 2), (2, 7, 2, 7), (1, -1, 1, 0), (1, 0, 1, -1), (1, I32_MIN, 1, I32_MAX),
          (1, I32_MAX, 1, I32_MIN), (3, -5, 2, -9), (2, -5, 3, -9), (-4, -7, -4, -7)]
    if name == "2int":
        ps += [(I32_MIN, 0, I32_MAX, 1), (I32_MAX, 0, I32_MIN, 1), (I32_MIN, 1, I32_MIN, 0), (I32_MAX, 5, I32_MAX, 5),
               (I32_MAX, 0, I32_MAX, -1), (I32_MIN, I32_MIN, I32_MIN, I32_MAX), (0, 1, -1, 0), (-1, 1, 0, 0)]
    else:
        ps += [(0.0, 3, -0.0, 3), (-0.0, 3, 0.0, 3), (0.0, 1, -0.0, 2), (-0.0, 1, 0.0, 2), (0.0, 2, -0.0, 1),
               (-0.0, 2, 0.0, 1), (inf, 1, -inf, 0), (-inf, 1, inf, 0), (inf, 4, inf, 2), (-inf, 1, -inf, 3),
               (inf, 0, 1.0, 0), (1.0, 0, -inf, 0), (nan, 0, 1.0, 1), (1.0, 0, nan, 1), (nan, 0, nan, 1),
               (nan, 1, nan, 0), (nan, 0, inf, 1), (-inf, 1, nan, 0), (nan, 3, nan, 3), (1.5, 0, 1.25, 1)]
    x, y = np.zeros(len(ps), dtype=ST[name]), np.zeros(len(ps), dtype=ST[name])
    for k, (xv, xi, yv, yi) in enumerate(ps):
        x["v"][k], x["i"][k], y["v"][k], y["i"][k] = xv, xi, yv, yi
    return x, y


def random_pairs(rng, n, name):
    """Values from a small set (many ties) mixed with random ones, indices in a small range
    (equal indices too), random padding."""
    a = np.zeros(n, dtype=ST[name])
    few = rng.integers(-3, 4, size=n)
    if name == "2int":
        wide = rng.integers(I32_MIN, I32_MAX, size=n, endpoint=True)
        a["v"] = np.where(rng.random(n) < 0.5, few, wide)
    else:
        a["v"] = np.where(rng.random(n) < 0.5, few * 0.5, rng.standard_normal(n) * 1e3)
    a["i"] = rng.integers(-4, 4, size=n)
    return fill_padding(a, rng)


# ---- children ------------------------------------------------------------------------
def run_child(cmd, env, timeout):
    """One child under a timeout; the test stops at the first one that fails."""
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def call(name, algo, op, inplace=0, offset=0, host=0):
    return {"dtype": name, "algo": algo, "op": op, "inplace": inplace, "offset": offset, "host": host}


def run_job(calls, inputs, p, env_extra=None, kills=(), timeout=120):
    """An ftrun job of p pair_worker ranks.  inputs[k][r]: rank r's structured vector of call k.
    Returns (completed process, out[k][r], status[k][r])."""
    tmp = tempfile.mkdtemp(prefix="ftar_pair_")
    try:
        json.dump(calls, open(os.path.join(tmp, "calls.json"), "w"))
        for k, per_rank in enumerate(inputs):
            for r, x in enumerate(per_rank):
                assert x.dtype == ST[calls[k]["dtype"]]
                raw(x).tofile(os.path.join(tmp, f"in_{r}_{k}.bin"))
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, PAIR_MODE="sched")
        env.pop("FTAR_KILL", None)
        if kills:
            env["FTAR_KILL"] = H.kill_env(kills)
        env.update(env_extra or {})
        cp = run_child([os.path.join(H.PKG, "bin", "ftrun"), "-np", str(p), "--devmap", ALL_ON_GPU0, sys.executable,
                        "-u", WORKER], env, timeout)
        outs, stats = [], []
        for k, c in enumerate(calls):
            o, s = {}, {}
            for r in range(p):
                f, g = os.path.join(tmp, f"out_{r}_{k}.bin"), os.path.join(tmp, f"status_{r}_{k}.txt")
                if os.path.exists(f) and os.path.exists(g):
                    o[r] = np.fromfile(f, dtype=np.uint8).view(ST[c["dtype"]])
                    s[r] = tuple(int(v) for v in open(g).read().split())
            outs.append(o)
            stats.append(s)
        return cp, outs, stats
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---- 1. local reduce -------------------------------------------------------------------
LOCAL_N = [0, 1, 2, 3, 5, 1031, 16397]
# (in, inout) byte offsets: aligned; a one-element head at 8 bytes (the 16-byte type: no vector
# body at all); operands that are not co-aligned; both 8 mod 16 from different distances
LOCAL_WINDOWS = [(0, 0), (8, 8), (8, 0), (0, 8), (24, 8)]


def _local_cases():
    cases = []
    for name in ST:
        tiles = 3 * 16384 // ST[name].itemsize + 5  # three 16 KiB tiles and a tail
        for op in OPS:
            cases += [dict(dtype=name, op=op, n=n, off_in=0, off_io=0, variant=1) for n in LOCAL_N]
            cases += [dict(dtype=name, op=op, n=16397, off_in=a, off_io=b, variant=1) for a, b in LOCAL_WINDOWS[1:]]
            cases += [dict(dtype=name, op=op, n=tiles, off_in=0, off_io=0, variant=v) for v in (0, 1)]
    return cases


def test_local_reduce_matrix():
    """ftar_reduce_local, three types x MAXLOC / MINLOC: sizes around the vector and the 16 KiB
    tile, windows at 8 mod 16 (a head of one 8-byte element; the 16-byte type on the scalar
    path) and operands that are not co-aligned, everything outside the window untouched, both
    local-reduce kernels; the first elements of every case are the special pairs.  One child
    runs the whole matrix."""
    cases = _local_cases()
    rng = np.random.default_rng(34)
    tmp = tempfile.mkdtemp(prefix="ftar_pair_local_")
    try:
        bufs = []
        for i, c in enumerate(cases):
            n, name = c["n"], c["dtype"]
            es = ST[name].itemsize
            x, y = random_pairs(rng, n, name), random_pairs(rng, n, name)  # x: inout, y: in
            sx, sy = special_pairs(name)
            m = min(n, sx.size)
            x[:m], y[:m] = fill_padding(sx, rng)[:m], fill_padding(sy, rng)[:m]
            a = rng.integers(0, 256, size=c["off_in"] + n * es + 48, dtype=np.uint8)
            b = rng.integers(0, 256, size=c["off_io"] + n * es + 48, dtype=np.uint8)
            a[c["off_in"]:c["off_in"] + n * es] = raw(y)
            b[c["off_io"]:c["off_io"] + n * es] = raw(x)
            a.tofile(os.path.join(tmp, f"lin_{i}.bin"))
            b.tofile(os.path.join(tmp, f"lio_{i}.bin"))
            bufs.append((a, b, x, y))
        json.dump(cases, open(os.path.join(tmp, "cases.json"), "w"))
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, PAIR_MODE="local")
        cp = run_child([sys.executable, "-u", WORKER], env, 120)
        assert cp.returncode == 0, cp.stderr[-3000:]
        status = [tuple(int(v) for v in ln.split()) for ln in open(os.path.join(tmp, "status.txt"))]
        assert len(status) == len(cases)
        for i, c in enumerate(cases):
            a, b, x, y = bufs[i]
            n, ob, name = c["n"], c["off_io"], c["dtype"]
            nb = n * ST[name].itemsize
            got = np.fromfile(os.path.join(tmp, f"lout_{i}.bin"), dtype=np.uint8)
            assert status[i] == (0, 1), (c, status[i])
            assert got.size == b.size
            assert np.array_equal(got[:ob], b[:ob]) and np.array_equal(got[ob + nb:], b[ob + nb:]), (c, "outside the window")
            assert_same_bytes(got[ob:ob + nb].view(ST[name]), loc(c["op"])(x, y), c)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---- 2. schedules against the oracle ---------------------------------------------------
ALL3, FD = ("float_int", "double_int", "2int"), ("float_int", "double_int")
TREE = {"FTAR_ONESHOT_MAX": "0"}
# (id, algo, p, bytes, settings, kill, element types): the rows of test_gpu_half.py's matrix,
# count = bytes / element size kept odd; float_int and double_int everywhere, 2int where the
# form is new ground for the type (one-shot, tree, step by step, push)
MATRIX = [
    ("oneshot_p8", "raben", 8, 2 * 4099, {}, None, ALL3),
    ("tree_p4", "raben", 4, 2 * 65541, TREE, None, ALL3),
    ("tree_u4_p4", "raben", 4, 2 * 65541, dict(TREE, FTAR_TREE_UNROLL="4"), None, FD),
    ("steps_p4", "raben", 4, 2 * 65541, {"FTAR_MESH": "0"}, None, ALL3),
    ("push_p4", "raben", 4, 2 * 65541, {"FTAR_PUSH": "2"}, None, ALL3),
    ("copy_engine_p4", "raben", 4, 2 * 65541, {"FTAR_COPY_ENGINE": "1", "FTAR_RELAY": "0", "FTAR_MESH": "0"}, None, FD),
    ("heads_p2", "raben", 2, None, {}, None, FD),  # count = 3
    ("prepost_p5", "raben", 5, 2 * 1031, {}, None, FD),
    # a death in reduce-scatter step 0 is fatal in the reference (raben/errhandler.c:37-38): the
    # oracle aborts and so must the job; the same victim point one step later recovers
    ("kill_step0_p5", "raben", 5, 2 * 1031, {}, (1, 1, 0, 1), FD),
    ("recovery_p5", "raben", 5, 2 * 1031, {}, (4, 1, 1, 1), FD),
    ("midexchange_p9", "raben", 9, 2 * 65541, {}, (5, 1, 1, 3), FD),
    ("rd_gated_p4", "rd", 4, 2 * 1031, {}, None, FD),
    ("rd_large_p4", "rd", 4, 2 * ((1 << 19) + 3), {}, None, FD),  # above the 1 MiB gate limit
    ("rd_recovery_p6", "rd", 6, 2 * 1031, {}, (3, 1, 1, 3), FD),
]
CASES = [pytest.param(*row[:6], name, id=f"{row[0]}-{name}") for row in MATRIX for name in row[6]]


def count_of(nbytes, name):
    if nbytes is None:
        return 3
    return nbytes // ST[name].itemsize | 1  # odd


def keyed_inputs(name, p, count, seed):
    """Rank r: values in [-8, 8] (many ties), index r * count + i, padding a function of the
    index (so the winner's padding is known from the decoded key)."""
    rng = np.random.default_rng(seed)
    ins = []
    for r in range(p):
        a = np.zeros(count, dtype=ST[name])
        a["v"] = rng.integers(-8, 9, size=count)
        a["i"] = r * count + np.arange(count)
        if "pad" in a.dtype.names:
            a["pad"] = pad_of(a["i"])
        ins.append(a)
    assert p * count < 2**31
    return ins


def pad_of(index):
    return ((index.astype(np.uint64) * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def keys_of(ins, op):
    out = []
    for a in ins:
        v, i = a["v"].astype(np.int64), a["i"].astype(np.int64)
        out.append(v * 2**32 + ((2**31 - 1 - i) if op == MAXLOC else i))
    return out


def decode(keys, op, name):
    a = np.zeros(keys.size, dtype=ST[name])
    low = keys & 0xFFFFFFFF
    a["v"] = keys >> 32
    a["i"] = (2**31 - 1 - low) if op == MAXLOC else low
    if "pad" in a.dtype.names:
        a["pad"] = pad_of(a["i"])
    return a


def check_against_oracle(oracle, name, algo, op, ins, kills, outs, stats, cp, what):
    fn = oracle.rabenseifner if algo == "raben" else oracle.recursive_doubling
    o = fn(keys_of(ins, op), kills, op=ORACLE_MAX if op == MAXLOC else ORACLE_MIN)
    if o.aborted:  # the outcome class is the oracle's: MPI_Abort, no rank returns
        assert "MPI_ABORT" in cp.stderr and not outs, (what, cp.stderr[-2000:])
        return o
    assert "MPI_ABORT" not in cp.stderr, (what, cp.stderr[-2000:])
    for w, st in enumerate(o.status):
        if st != 0:
            assert w not in outs, (what, "rank", w, "died in the oracle")
            continue
        assert w in outs, (what, "rank", w, cp.stderr[-2000:])
        rc, size_after, recoveries, intact = stats[w]
        assert (rc, size_after, recoveries) == (o.ret, len(o.order_after), o.recoveries), (what, w, stats[w])
        assert intact == 1, (what, w, "guards or send buffer written")
        assert_same_bytes(outs[w], decode(o.outputs[w], op, name), (what, "rank", w))
    return o


@pytest.mark.parametrize("cid,algo,p,nbytes,settings,kill,name", CASES)
def test_schedule_against_oracle(oracle, cid, algo, p, nbytes, settings, kill, name):
    """MAXLOC and MINLOC through one form of a schedule: two calls of one job without a kill,
    one job per op with one; return code, comm size after the call, recoveries and the
    aborted / died outcome are the oracle's too."""
    count = count_of(nbytes, name)
    ins = {op: keyed_inputs(name, p, count, seed=2000 + 10 * p + op) for op in OPS}
    if kill:
        for op in OPS:
            cp, outs, stats = run_job([call(name, algo, op)], [ins[op]], p, settings, [kill])
            o = check_against_oracle(oracle, name, algo, op, ins[op], [kill], outs[0], stats[0], cp, (cid, name, op))
            assert o.aborted == (cid == "kill_step0_p5") and (o.aborted or o.recoveries == 1), (cid, o.aborted, o.recoveries)
        return
    cp, outs, stats = run_job([call(name, algo, op) for op in OPS], [ins[op] for op in OPS], p, settings)
    assert cp.returncode == 0, cp.stderr[-3000:]
    for k, op in enumerate(OPS):
        check_against_oracle(oracle, name, algo, op, ins[op], [], outs[k], stats[k], cp, (cid, name, op))


def test_inplace_and_offset(oracle):
    """sbuf == rbuf and windows at byte offset 8 (a one-element head for the 8-byte types, the
    scalar path for the 16-byte type) at p = 4: the tree form in one job, the one-shot and gated
    recursive-doubling forms in another; the 8-byte types' windows at 4 and 12 in a third."""
    calls = [call("float_int", "raben", MAXLOC, inplace=1), call("double_int", "raben", MINLOC, offset=8),
             call("double_int", "rd", MAXLOC, inplace=1, offset=8), call("2int", "rd", MINLOC, offset=8)]
    data = [keyed_inputs(c["dtype"], 4, count_of(2 * 65541, c["dtype"]), seed=60 + k) for k, c in enumerate(calls)]
    cp, outs, stats = run_job(calls, data, 4, TREE)
    assert cp.returncode == 0, cp.stderr[-3000:]
    for k, c in enumerate(calls):
        check_against_oracle(oracle, c["dtype"], c["algo"], c["op"], data[k], [], outs[k], stats[k], cp, ("device", k))
    # the same windows at one-shot size: the gated launches stage the input element by element
    # where it is not 16-byte aligned (16-byte elements as two 8-byte halves)
    calls = [call("double_int", "raben", MAXLOC, offset=8), call("double_int", "rd", MINLOC, offset=8),
             call("float_int", "raben", MINLOC, offset=8), call("2int", "rd", MAXLOC, inplace=1, offset=8)]
    data = [keyed_inputs(c["dtype"], 4, count_of(2 * 4099, c["dtype"]), seed=80 + k) for k, c in enumerate(calls)]
    cp, outs, stats = run_job(calls, data, 4)
    assert cp.returncode == 0, cp.stderr[-3000:]
    for k, c in enumerate(calls):
        check_against_oracle(oracle, c["dtype"], c["algo"], c["op"], data[k], [], outs[k], stats[k], cp, ("small", k))
    # the alignment the header allows the 8-byte pair types: windows 4 and 12 bytes past a 16-byte
    # boundary -- co-aligned, yet no element sits on a vector boundary: the scalar path.  Both
    # types at the one-shot size (its gated launch stages the unaligned input element by element)
    # and at the tree size, in one job with the one-shot limit between the two
    calls = [call("float_int", "raben", MINLOC, offset=4), call("2int", "raben", MAXLOC, offset=12),
             call("2int", "raben", MINLOC, offset=4), call("float_int", "raben", MAXLOC, inplace=1, offset=12)]
    sizes = [2 * 4099, 2 * 4099, 2 * 65541, 2 * 65541]
    data = [keyed_inputs(c["dtype"], 4, count_of(sizes[k], c["dtype"]), seed=90 + k) for k, c in enumerate(calls)]
    cp, outs, stats = run_job(calls, data, 4, {"FTAR_ONESHOT_MAX": str(64 << 10)})
    assert cp.returncode == 0, cp.stderr[-3000:]
    for k, c in enumerate(calls):
        check_against_oracle(oracle, c["dtype"], c["algo"], c["op"], data[k], [], outs[k], stats[k], cp, ("4 mod 8", k))


def test_host_buffers(oracle):
    """The *_host entry points on pageable buffers (H2D, device Allreduce, D2H), p = 2, one job."""
    calls = [call("float_int", "raben", MAXLOC, host=1), call("double_int", "rd", MAXLOC, host=1),
             call("double_int", "raben", MINLOC, host=1, offset=8), call("2int", "rd", MINLOC, host=1, offset=8)]
    data = [keyed_inputs(c["dtype"], 2, count_of(2 * 4099, c["dtype"]), seed=70 + k) for k, c in enumerate(calls)]
    cp, outs, stats = run_job(calls, data, 2)
    assert cp.returncode == 0, cp.stderr[-3000:]
    for k, c in enumerate(calls):
        check_against_oracle(oracle, c["dtype"], c["algo"], c["op"], data[k], [], outs[k], stats[k], cp, ("host", k))


# ---- 3. real comparisons through the trees ---------------------------------------------
def real_inputs(name, p, count, seed):
    """Random finite values, about 1/8 of the elements holding one value on several ranks.  At
    every element the ranks' indices are a permutation of -p/2 .. p/2 - 1: equal values meet
    lower and higher indices but never an equal one, so the winner does not depend on the
    operand order and recursive doubling's ranks, each with its own order, must agree (the
    equal pair, where y's bytes win, is section 1's).  Random padding."""
    rng = np.random.default_rng(seed)
    shared = rng.standard_normal(count) * 100
    dup = rng.random(count) < 0.125
    index = np.argsort(rng.random((p, count)), axis=0) - p // 2
    ins = []
    for r in range(p):
        a = np.zeros(count, dtype=ST[name])
        a["v"] = np.where(dup & (rng.random(count) < 0.6), shared, rng.standard_normal(count) * 100)
        a["i"] = index[r]
        assert np.all(np.isfinite(a["v"]))
        ins.append(fill_padding(a, rng))
    return ins


TREES = [(form, algo, settings, p) for form, algo, settings in
         (("raben", "raben", {}), ("raben_steps", "raben", {"FTAR_MESH": "0"}), ("rd", "rd", {})) for p in (2, 4, 8)]


@pytest.mark.parametrize("form,algo,settings,p", TREES, ids=[f"{t[0]}-p{t[3]}" for t in TREES])
def test_schedule_trees(form, algo, settings, p):
    """No kills: float_int and double_int, MAXLOC and MINLOC as four calls of one job, against
    half_model.py's trees (validated against the oracle in test_half_abi.py) with the pairwise
    rule at every node; all ranks agree byte for byte."""
    count = 1031 if p == 2 else 4099
    calls = [call(name, algo, op) for name in FD for op in OPS]
    data = [real_inputs(c["dtype"], p, count, seed=300 + 10 * p + k) for k, c in enumerate(calls)]
    cp, outs, stats = run_job(calls, data, p, settings)
    assert cp.returncode == 0, (form, p, cp.stderr[-3000:])
    for k, c in enumerate(calls):
        assert sorted(outs[k]) == list(range(p)), (form, p, k, cp.stderr[-2000:])
        want = M.raben_tree(data[k], loc(c["op"])) if algo == "raben" else M.rd_tree(data[k], loc(c["op"]))[0]
        for w in range(p):
            assert stats[k][w][0] == 0 and stats[k][w][3] == 1, (form, p, k, w, stats[k][w])
            assert_same_bytes(outs[k][w], outs[k][0], (form, p, k, "ranks", w, "and 0 differ"))
            assert_same_bytes(outs[k][w], want, (form, p, k, "rank", w))
