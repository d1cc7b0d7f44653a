"""The 8-, 16-bit and unsigned integer types (FTAR_INT8 = 48 .. FTAR_UINT64 = 53) on the GPU: the
local reduce, the kernels alone, both Allreduce schedules with and without kills, the list entry
point, the host entry points and the Python binding -- byte for byte.

Every GPU action runs in a child under its own timeout (tests/int_worker.py directly or as the
ranks of an ftrun job, all on GPU 0; tests/int_types/_build/int_check); a test stops at the first
child that fails; the pytest process never opens the GPU.

References
* local reduce: tests/int_types/ref_check's plain C++ `apply` (pinned to numpy on the CPU by
  test_int_ref.py), on every 8-bit operand pair and on every 16-bit pattern against 48 partners;
* kernels alone: int_check compares with the same reference itself;
* schedules without kills: numpy's reduce over the ranks (int_model.reduce_ranks) -- every op is
  exactly associative and commutative on these types, so every form gives these bytes;
* schedules with kills: the unchanged oracle, which knows int64, on mapped values
  (int_model.to_oracle / from_oracle; test_int_ref.py shows the maps commute with every op).
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import harness as H
import int_model as I

pytestmark = pytest.mark.gpu

ALL_ON_GPU0 = ",".join(["0"] * 16)
WORKER = os.path.join(H.ROOT, "tests", "int_worker.py")
DIR = os.path.join(H.ROOT, "tests", "int_types", "_build")
ES = {dt: np.dtype(t).itemsize for dt, t in I.NP.items()}
# the (type, op) pairs of the schedule tests: wrap-around sums and products, compares in each
# signedness with values on both sides of 2^(w-1), a bitwise op
COMBOS = [(I.INT8, I.SUM), (I.UINT8, I.MAX), (I.UINT8, I.BOR), (I.INT16, I.PROD), (I.UINT16, I.MIN), (I.UINT32, I.MAX),
          (I.UINT64, I.MIN)]


def run_child(cmd, env, timeout):
    """One child under a timeout; the test stops at the first one that fails."""
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def call(dt, algo, op, inplace=0, offset=0, host=0):
    return {"dtype": dt, "es": ES[dt], "algo": algo, "op": op, "inplace": inplace, "offset": offset, "host": host}


def run_job(calls, inputs, p, env_extra=None, kills=(), timeout=120, mode="sched"):
    """An ftrun job of p int_worker ranks.  inputs[k][r]: rank r's vector of call k.
    Returns (completed process, out[k][r], status[k][r])."""
    tmp = tempfile.mkdtemp(prefix="ftar_int_")
    try:
        json.dump(calls, open(os.path.join(tmp, "calls.json"), "w"))
        for k, per_rank in enumerate(inputs):
            for r, x in enumerate(per_rank):
                assert x.dtype == I.NP[calls[k]["dtype"]]
                I.raw(x).tofile(os.path.join(tmp, f"in_{r}_{k}.bin"))
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, INT_MODE=mode)
        env.pop("FTAR_KILL", None)
        if kills:
            env["FTAR_KILL"] = H.kill_env(kills)
        env.update(env_extra or {})
        cp = run_child([os.path.join(H.PKG, "bin", "ftrun"), "-np", str(p), "--devmap", ALL_ON_GPU0, sys.executable, "-u", WORKER],
                       env, timeout)
        outs, stats = [], []
        for k, c in enumerate(calls):
            o, s = {}, {}
            for r in range(p):
                f, g = os.path.join(tmp, f"out_{r}_{k}.bin"), os.path.join(tmp, f"status_{r}_{k}.txt")
                if os.path.exists(f) and os.path.exists(g):
                    o[r] = np.fromfile(f, dtype=I.NP[c["dtype"]])
                    s[r] = tuple(int(v) for v in open(g).read().split())
            outs.append(o)
            stats.append(s)
        return cp, outs, stats
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def full_range(rng, dt, n):
    """Uniform over all 2^w patterns: both sides of 2^(w-1) in either signedness."""
    w = 8 * ES[dt]
    return rng.integers(0, 1 << w, size=n, dtype=np.uint64, endpoint=False).astype({8: np.uint8, 16: np.uint16, 32: np.uint32,
                                                                                     64: np.uint64}[w]).view(I.NP[dt])


# ---- 1. local reduce -------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_check():
    exe = os.path.join(DIR, "ref_check")
    assert os.path.exists(exe), "tests/int_types is not built (python -c 'import __graft_entry__ as g; g.build()')"
    return exe


def _local_cases():
    """(case, operand key).  8-bit: every operand pair, all ten ops, both signednesses, both
    kernels.  16-bit: the pattern vector, uint16 all ten ops and int16's own MAX / MIN (and SUM,
    through the dispatch), both kernels.  Then windows at 1, 7 and 15 elements with lengths that
    leave tails of 1 and 15 elements (two ops each, the ops and the two kernels in turn), one pair
    of operands that is not co-aligned, the 32- and 64-bit unsigned types, one case on pinned host
    memory."""
    cases = []

    def add(dt, op, n, off_in, off_io, variant, pinned=0):
        cases.append(dict(dtype=dt, es=ES[dt], op=op, n=n, off_in=off_in * ES[dt], off_io=off_io * ES[dt], variant=variant,
                          pinned=pinned))

    for dt in (I.INT8, I.UINT8, I.INT16, I.UINT16):
        whole = (1 << 16) if ES[dt] == 1 else (48 << 16)
        ops = I.OPS if dt != I.INT16 else (I.SUM, I.MAX, I.MIN)
        for op in ops:
            for v in (0, 1):
                add(dt, op, whole, 0, 0, v)
        k = 0
        for off in (1, 7, 15):
            for tail in (1, 15):
                for _ in range(2):
                    add(dt, I.OPS[k % 10], 2 * 16384 // ES[dt] + 16 + tail, off, off, k & 1)
                    k += 1
        add(dt, I.MAX, 4099, 1, 0, 0)  # not co-aligned: the scalar path
    for dt in (I.UINT32, I.UINT64):
        n = I.operands(dt)[0].size
        for op in I.OPS:
            for v in (0, 1):
                add(dt, op, n, 0, 0, v)
        add(dt, I.MAX, n - 3, 1, 1, 0)
        add(dt, I.MIN, n - 3, 1, 1, 0)
    add(I.UINT8, I.SUM, 1 << 16, 0, 0, 1, pinned=1)
    add(I.INT8, I.MIN, (1 << 16) - 17, 15, 15, 0, pinned=1)
    return cases


def test_local_reduce(ref_check):
    """ftar_reduce_local against the plain reference: one child runs the whole matrix on operand
    files shared per type; everything outside the window untouched, `in` untouched."""
    cases = _local_cases()
    tmp = tempfile.mkdtemp(prefix="ftar_int_local_")
    try:
        ops, want = {}, {}
        for dt in I.TYPES:
            x, y = I.operands(dt)  # x: inout, y: in
            ops[dt] = (x, y)
            for which, a in (("io", x), ("in", y)):
                buf = np.concatenate([I.raw(a), np.full(64, 0x77, dtype=np.uint8)])
                buf.tofile(os.path.join(tmp, f"{which}_{dt}.bin"))
        for i, c in enumerate(cases):  # the worker reads lin_i / lio_i: links to the type's files
            os.symlink(os.path.join(tmp, f"in_{c['dtype']}.bin"), os.path.join(tmp, f"lin_{i}.bin"))
            os.symlink(os.path.join(tmp, f"io_{c['dtype']}.bin"), os.path.join(tmp, f"lio_{i}.bin"))
        json.dump(cases, open(os.path.join(tmp, "cases.json"), "w"))
        cp = run_child([sys.executable, "-u", WORKER], dict(os.environ, FTAR_PROBE_DIR=tmp, INT_MODE="local"), 240)
        assert cp.returncode == 0, cp.stderr[-3000:]
        status = [tuple(int(v) for v in ln.split()) for ln in open(os.path.join(tmp, "status.txt"))]
        assert len(status) == len(cases)
        for i, c in enumerate(cases):
            dt, es, n, oi, oo = c["dtype"], c["es"], c["n"], c["off_in"], c["off_io"]
            x, y = ops[dt]
            xin, yin = I.raw(x)[oo:oo + n * es].view(I.NP[dt]), I.raw(y)[oi:oi + n * es].view(I.NP[dt])
            key = (dt, c["op"], n, oi, oo)
            if key not in want:  # the reference program, once per distinct window
                fi, fio, fo = (os.path.join(tmp, f) for f in ("r_in.bin", "r_io.bin", "r_out.bin"))
                yin.tofile(fi)
                xin.tofile(fio)
                rc = run_child([ref_check, "apply", str(dt), str(c["op"]), fi, fio, fo], None, 120)
                assert rc.returncode == 0, rc.stderr[-2000:]
                want[key] = np.fromfile(fo, dtype=I.NP[dt])
            got = np.fromfile(os.path.join(tmp, f"lout_{i}.bin"), dtype=np.uint8)
            whole = np.fromfile(os.path.join(tmp, f"io_{dt}.bin"), dtype=np.uint8)
            assert status[i] == (0, 1), (c, status[i])
            assert got.size == whole.size
            assert np.array_equal(got[:oo], whole[:oo]) and np.array_equal(got[oo + n * es:], whole[oo + n * es:]), (c, "outside the window")
            assert_same(got[oo:oo + n * es].view(I.NP[dt]), want[key], c)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---- 2. kernels alone ------------------------------------------------------------------
def _int_check(args, timeout):
    exe = os.path.join(DIR, "int_check")
    assert os.path.exists(exe), "tests/int_types is not built"
    cp = run_child([exe] + args, None, timeout)
    assert cp.returncode == 0, cp.stdout[-4000:] + cp.stderr[-2000:]
    last = cp.stdout.rstrip().splitlines()[-1]
    assert last.startswith("int_check: ") and last.endswith(" 0 failed") and int(last.split()[1]) > 1000, last
    print(last)


def test_kernels_alone():
    """segment_kernel (reduce, copy, two outputs), tree_kernel (P = 2 .. 16, U = 1, 2, 4),
    tree_batch_kernel (P = 2, 4, 8), reduce_lds_kernel and the mover: every new (T, OP) pair, every
    window offset, lengths 5, 31 and a tile + 16 + 3 (int_check.hip lists the cases)."""
    _int_check([], 240)


@pytest.mark.parametrize("wide", H.wide("wide"))
def test_kernels_alone_every_type_and_op(wide):
    _int_check([wide], 600)


# ---- 3. schedules without faults -------------------------------------------------------
COUNTS = [1, 15, 17, 4099, 2 * 65541]  # 4099: halving lands on odd bytes; 2 x 65541 bytes of int8: past the one-shot limit
MESH0, PUSH1, PUSH2 = {"FTAR_MESH": "0"}, {"FTAR_PUSH": "1"}, {"FTAR_PUSH": "2"}
RELAY = {"FTAR_RELAY_MIN": "0", "FTAR_MESH": "0"}
COPY_ENGINE = {"FTAR_COPY_ENGINE": "1", "FTAR_RELAY": "0", "FTAR_MESH": "0"}
FORMS = [("raben", "default", {}, p) for p in (2, 4, 8)] + [("rd", "default", {}, p) for p in (2, 4, 8)] + \
        [("raben", "mesh0", MESH0, p) for p in (2, 4, 8)] + [("raben", "push2", PUSH2, p) for p in (2, 4, 8)] + \
        [("raben", "push1", PUSH1, p) for p in (2, 4, 8)] + [("raben", "relay", RELAY, p) for p in (2, 4, 8)] + \
        [("raben", "copy_engine", COPY_ENGINE, p) for p in (2, 4, 8)] + H.wide(("rd", "copy_engine", COPY_ENGINE, 4))


ONESHOT_64K = {"FTAR_ONESHOT_MAX": str(64 << 10)}  # the counts up to 4099 one-shot, 2 x 65541 past the limit at every size


def _no_fault(calls, data, p, settings, what):
    cp, outs, stats = run_job(calls, data, p, settings, timeout=240)
    assert cp.returncode == 0, (what, cp.stderr[-3000:])
    for k, c in enumerate(calls):
        assert sorted(outs[k]) == list(range(p)), (what, k, cp.stderr[-2000:])
        want = I.reduce_ranks(data[k], c["op"])
        for w in range(p):
            assert stats[k][w][:4] == (0, p, 0, 1), (what, k, w, stats[k][w])
            assert_same(outs[k][w], want, (what, I.NAMES[c["dtype"]], I.OP_NAMES[c["op"]], data[k][0].size, "rank", w))


@pytest.mark.parametrize("algo,form,settings,p", FORMS, ids=[f"{f[0]}-{f[1]}-p{f[3]}" for f in FORMS])
def test_schedule_forms(algo, form, settings, p):
    """One job per form: the seven (type, op) pairs x the five counts, the last call of each pair
    in place and the one before at an odd byte offset (1-byte types) or one element in.  The one-shot
    limit is set to 64 KiB, so that the largest count takes the form's own path (tree, steps, push)
    at every element size and the others the one-shot launch."""
    rng = np.random.default_rng(4800 + 10 * p + len(form))
    calls, data = [], []
    for dt, op in COMBOS:
        for j, n in enumerate(COUNTS):
            calls.append(call(dt, algo, op, inplace=int(j == 4), offset=ES[dt] if j == 3 else 0))
            data.append([full_range(rng, dt, n) for _ in range(p)])
    _no_fault(calls, data, p, dict(ONESHOT_64K, **settings), (algo, form, p))


def test_every_type_and_op_p4():
    """The whole op x type matrix, Rabenseifner's default form at p = 4, count 4099, one job."""
    rng = np.random.default_rng(53)
    calls = [call(dt, "raben", op) for dt in I.TYPES for op in I.OPS]
    data = [[full_range(rng, c["dtype"], 4099) for _ in range(4)] for c in calls]
    for k, c in enumerate(calls):  # zeros too, for the logical ops
        if c["op"] in (I.LAND, I.LOR, I.LXOR):
            for x in data[k]:
                x[rng.random(x.size) < 0.5] = 0
    _no_fault(calls, data, 4, {}, "matrix")


@pytest.mark.parametrize("p", [2, 4, 8])
def test_default_settings_past_a_tile(p):
    """The product's own settings, nothing overridden (the one-shot limit at its default): the seven
    pairs at 2 x 65541 elements through both schedules, one job per size."""
    rng = np.random.default_rng(5300 + p)
    calls = [call(dt, algo, op) for dt, op in COMBOS for algo in ("raben", "rd")]
    data = [[full_range(rng, c["dtype"], 2 * 65541) for _ in range(p)] for c in calls]
    _no_fault(calls, data, p, {}, ("defaults", p))


# ---- 4. schedules with kills, against the unchanged oracle -----------------------------
# (p, kill): one in the reduce-scatter loop, one in the allgather, one mid-exchange, per size
KILLS = [(5, (4, 1, 1, 1)), (5, (3, 2, 0, 1)), (5, (3, 1, 1, 3)),
         (6, (5, 1, 1, 1)), (6, (4, 2, 0, 1)), (6, (3, 1, 1, 3)),
         (9, (6, 1, 1, 1)), (9, (6, 2, 1, 1)), (9, (6, 1, 1, 3))]


def kill_inputs(rng, dt, op, p, n):
    """Full range, but PROD (on int16 here): factors of magnitude 20 .. 100, so that the exact
    product of the four to nine ranks' values fits int64 (100^9 = 10^18 < 2^63) but not 16 bits
    (20^4 > 2^17): the truncation modulo 2^w is exercised and the oracle's own arithmetic never
    wraps."""
    if op != I.PROD:
        return [full_range(rng, dt, n) for _ in range(p)]
    assert dt in (I.INT16, I.UINT16) and p <= 9
    signed = np.dtype(I.NP[dt]).kind == "i"
    out = []
    for _ in range(p):
        v = rng.integers(20, 101, size=n)
        if signed:
            v = v * rng.choice([-1, 1], size=n)
        out.append(v.astype(I.NP[dt]))
    return out


@pytest.mark.parametrize("j,p,kill", [(j, p, k) for j, (p, k) in enumerate(KILLS)], ids=[f"p{p}-" + "_".join(map(str, k)) for p, k in KILLS])
def test_schedule_with_kill(oracle, j, p, kill):
    """One Rabenseifner job with one kill; the (type, op) pairs take turns over the kills.  Every
    survivor's bytes, return code, recoveries and comm size after the call are the oracle's, and so
    is the outcome class (a kill the reference cannot recover from aborts the job)."""
    dt, op = COMBOS[j % len(COMBOS)]
    n = 2 * 1031 + 1
    ins = kill_inputs(np.random.default_rng(900 + j), dt, op, p, n)
    cp, outs, stats = run_job([call(dt, "raben", op)], [ins], p, {}, [kill], timeout=180)
    o = oracle.rabenseifner([I.to_oracle(x, dt, op) for x in ins], [kill], op=op)
    what = (I.NAMES[dt], I.OP_NAMES[op], p, kill)
    if op == I.PROD:  # the premise of the map: the oracle's int64 products cannot wrap
        assert max(int(np.abs(x.astype(np.int64)).max()) for x in ins) ** p < 2 ** 63, what
    if o.aborted:
        assert "MPI_ABORT" in cp.stderr and not outs[0], (what, cp.stderr[-2000:])
        return
    assert "MPI_ABORT" not in cp.stderr, (what, cp.stderr[-2000:])
    assert o.recoveries >= 1, (what, "the kill was not noticed by the oracle")
    for w, st in enumerate(o.status):
        if st != 0:
            assert w not in outs[0], (what, "rank", w, "died in the oracle")
            continue
        assert w in outs[0], (what, "rank", w, cp.stderr[-2000:])
        rc, size_after, recoveries, intact = stats[0][w][:4]
        assert (rc, size_after, recoveries) == (o.ret, len(o.order_after), o.recoveries), (what, w, stats[0][w])
        assert intact == 1, (what, w, "guards or send buffer written")
        assert_same(outs[0][w], I.from_oracle(o.outputs[w], dt, op), (what, "rank", w))


# ---- 5. lists ----------------------------------------------------------------------------
def test_list_of_uint8_buffers():
    """ftar_allreduce_multi on 7 uint8 buffers of 1, 3, 16, 17, 4099, 0 and 33 elements at odd
    addresses, the 17-element one in place: the bytes of the plain call on the concatenation (the
    job's second call), coalesced == 6, nothing outside the output windows written.  On the same
    list ftar_allreduce_multi_acc32 keeps its codes: MPI_ERR_ARG for the dtype, MPI_ERR_OP for
    MAXLOC (the op / dtype check comes first)."""
    sizes = [1, 3, 16, 17, 4099, 0, 33]
    lst, at = [], 1
    for n in sizes:
        lst.append([at, n, int(n == 17)])
        at += n + (2 if (at + n) % 2 else 1)  # the next entry at an odd address again
    assert all(off % 2 == 1 for off, _, _ in lst)
    rng = np.random.default_rng(61)
    p, total = 4, sum(sizes)
    data = [full_range(rng, I.UINT8, total) for _ in range(p)]
    for algo in ("raben", "rd"):
        listed = dict(call(I.UINT8, algo, I.SUM), list=lst)
        cp, outs, stats = run_job([listed, call(I.UINT8, algo, I.SUM)], [data, data], p, timeout=120)
        assert cp.returncode == 0, (algo, cp.stderr[-3000:])
        want = I.reduce_ranks(data, I.SUM)
        for w in range(p):
            assert stats[0][w] == (0, p, 0, 1, 6, 13, 9), (algo, w, stats[0][w])
            assert stats[1][w][:4] == (0, p, 0, 1), (algo, w, stats[1][w])
            assert_same(outs[0][w], outs[1][w], (algo, "list and plain call differ", w))
            assert_same(outs[0][w], want, (algo, "rank", w))


# ---- 6. host entry points and the Python binding -------------------------------------------
def test_host_entry_points_int16():
    """One _host call per algo on int16 (pageable buffers: H2D, device Allreduce, D2H), p = 2."""
    rng = np.random.default_rng(71)
    calls = [call(I.INT16, "raben", I.PROD, host=1), call(I.INT16, "rd", I.MIN, host=1, offset=2)]
    data = [[full_range(rng, I.INT16, 4099) for _ in range(2)] for _ in calls]
    _no_fault(calls, data, 2, {}, "host")


def test_host_pipeline_chunks_every_op():
    """ftar_allreduce_rabenseifner_host on pageable buffers of 16 MiB + 4099 bytes, p = 2: from 16 MiB
    on the vector goes through as a pipeline of chunk Allreduces where the op commutes exactly --
    on these types every op does, MAX and a bitwise op here (`commutes`, ftar_raben.c).  Chunking
    moves the block boundaries; the bytes must not move."""
    rng = np.random.default_rng(73)
    n = (16 << 20) + 4099
    calls = [call(I.UINT8, "raben", I.MAX, host=1), call(I.INT8, "raben", I.BXOR, host=1, offset=1)]
    data = [[full_range(rng, c["dtype"], n) for _ in range(2)] for c in calls]
    _no_fault(calls, data, 2, {"FTAR_HOST_PIPE": "1"}, "host pipeline")


def test_torch_uint8_tensor():
    """A torch.uint8 CUDA tensor through Comm.allreduce_rabenseifner, the dtype taken from the
    tensor: BOR of flag bytes, p = 2.  Then a torch.int16 tensor, which the binding does not map
    (the storage view of raw 2-byte float bits), with dtype=INT16 named by the caller: MIN."""
    rng = np.random.default_rng(72)
    calls = [call(I.UINT8, "raben", I.BOR), call(I.INT16, "raben", I.MIN)]
    data = [[full_range(rng, I.UINT8, 4099) & np.uint8(1 << r | 0x10) for r in range(2)],
            [full_range(rng, I.INT16, 4099) for r in range(2)]]
    cp, outs, stats = run_job(calls, data, 2, mode="torch", timeout=300)
    assert cp.returncode == 0, cp.stderr[-3000:]
    for k, c in enumerate(calls):
        want = I.reduce_ranks(data[k], c["op"])
        for w in range(2):
            assert stats[k][w][:3] == (0, 2, 0), (k, w, stats[k][w])
            assert_same(outs[k][w], want, ("torch", k, w))
