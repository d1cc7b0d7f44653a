"""ftar_allreduce_multi_mixed (test infrastructure): the numpy model of the call's definition, and
jobs of tests/mixed/mixed_probe.c under ftrun against libftar.so, every rank on GPU 0.

The model, numpy only.  A list is (counts, types): types[i] the ftar_dtype of entry i (1: float32,
16: float16, 17: bfloat16).  A rank's data is the list's bytes, entry after entry, as one uint8
vector ("raw"); `widen_list` turns it into the dense float32 vector the schedule sees (per entry
acc32_runner.widen, a float32 entry as it is), `narrow_list` is the way back (per entry
acc32_runner.narrow).

    expected = narrow_list(np.float32(scale) * oracle_fn(widen_list(inputs), kills, op).outputs[w])

`same` compares two raw vectors through their widened values (widening is exact and injective, so
this is bit equality) with multi_runner.same_bits_or_nan: a NaN of any payload exactly where the
model holds one, every other element bit for bit.
"""
from __future__ import annotations

import fcntl
import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass

import numpy as np

import acc32_runner as A
import harness as H
import multi_runner as R

DIR = os.path.join(H.ROOT, "tests", "mixed")
F32, F16, BF16 = 1, A.F16, A.BF16
CYCLE = (BF16, F32, F16)  # neighbours differ
HBM = A.HBM
NAN_CAP = 0.25


def esize(dt) -> int:
    return 4 if dt == F32 else 2


def cycle(n, start=0):
    return [CYCLE[(i + start) % 3] for i in range(n)]


def nbytes(counts, types) -> int:
    return sum(c * esize(t) for c, t in zip(counts, types))


def pieces(counts, types):
    """[(type, first byte, first element, count)] of the non-empty entries."""
    out, b, e = [], 0, 0
    for c, t in zip(counts, types):
        if c:
            out.append((t, b, e, c))
        b += c * esize(t)
        e += c
    return out


def widen_list(raw, counts, types) -> np.ndarray:
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    assert raw.size == nbytes(counts, types)
    out = np.empty(sum(counts), dtype=np.float32)
    for t, b, e, c in pieces(counts, types):
        seg = raw[b:b + c * esize(t)]
        out[e:e + c] = seg.view(np.float32) if t == F32 else A.widen(seg.view(np.uint16), t)
    return out


def narrow_list(f32, counts, types) -> np.ndarray:
    f32 = np.ascontiguousarray(f32, dtype=np.float32)
    assert f32.size == sum(counts)
    out = np.empty(nbytes(counts, types), dtype=np.uint8)
    for t, b, e, c in pieces(counts, types):
        seg = f32[e:e + c]
        out[b:b + c * esize(t)] = (seg if t == F32 else A.narrow(seg, t)).view(np.uint8)
    return out


def model(fn, raws, counts, types, op, scale, kills=()):
    """(the oracle's Result on the widened inputs, [rank -> expected raw vector])."""
    o = fn([widen_list(x, counts, types) for x in raws], list(kills), op=op)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return o, [narrow_list(np.float32(scale) * y, counts, types) for y in o.outputs]


def same(got, want, counts, types) -> bool:
    return got.size == want.size and R.same_bits_or_nan(widen_list(got, counts, types), widen_list(want, counts, types))


def nan_share(raw, counts, types) -> float:
    return float(np.mean(np.isnan(widen_list(raw, counts, types))))


def specials(oracle, p, counts, types, seed):
    """Random inputs with NaN, +-0 and +-inf (H.with_specials on float32 values), every entry
    narrowed to its own type, so every value is representable."""
    f = H.with_specials(oracle.random_inputs(p, sum(counts), seed=seed, dtype=np.float32), seed)
    return [narrow_list(x, counts, types) for x in f]


def build() -> str:
    """The probe, one build at a time."""
    with open(os.path.join(H.ROOT, "tests", "hostsim", ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", DIR, "gpu"], check=True)
    return os.path.join(DIR, "_build", "gpu", "mixed_probe")


@dataclass
class MixedRun:
    returncode: int
    stderr: str
    outputs: list  # [call][rank] -> raw result, uint8
    status: list   # [call][rank] -> status tuple
    plain: list    # [call][rank] -> the plain FLOAT32 entry point's result, float32

    @property
    def aborted(self) -> bool:
        return "MPI_ABORT" in self.stderr


def run_mixed(algo, calls, p, op=0, scale=1.0, mode=0, kills=(), inplace=0, offset=0, plain=False, env_extra=None,
              timeout=90) -> MixedRun:
    """calls: [(counts, types, [rank r's raw vector])]; op, scale and mode: one value, or a list with
    one per call.  plain=True: the probe also runs the plain FLOAT32 entry point on the widened
    vector, which this function supplies as a second input file."""
    tmp = tempfile.mkdtemp(prefix="ftar_mixed_")
    try:
        for k, (counts, types, ins) in enumerate(calls):
            assert len(ins) == p and len(counts) == len(types)
            for r, x in enumerate(ins):
                x = np.ascontiguousarray(x)
                assert x.dtype == np.uint8 and x.size == nbytes(counts, types)
                x.tofile(os.path.join(tmp, f"in_{r}_{k}.bin"))
                if plain:
                    widen_list(x, counts, types).tofile(os.path.join(tmp, f"in32_{r}_{k}.bin"))
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, FTAR_PROBE_ALGO=algo, FTAR_PROBE_OP=A._semi(op),
                   FTAR_MIXED_SCALE=A._semi([float(x) for x in scale] if isinstance(scale, (list, tuple)) else float(scale)),
                   FTAR_MIXED_MODE=A._semi(mode),
                   FTAR_MULTI_COUNTS=";".join(",".join(str(c) for c in counts) for counts, _, _ in calls),
                   FTAR_MIXED_TYPES=";".join(",".join(str(t) for t in types) for _, types, _ in calls),
                   FTAR_PROBE_INPLACE=str(inplace), FTAR_PROBE_OFFSET=str(offset), FTAR_MIXED_PLAIN=str(int(plain)))
        env.pop("FTAR_KILL", None)
        if kills:
            env["FTAR_KILL"] = H.kill_env(kills)
        env.update(env_extra or {})
        cmd = [os.path.join(H.PKG, "bin", "ftrun"), "-np", str(p), "--devmap", R.ALL_ON_GPU0,
               os.path.join(DIR, "_build", "gpu", "mixed_probe")]
        cp = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
        outs, stats, plains = [], [], []
        for k in range(len(calls)):
            o, s, q = {}, {}, {}
            for r in range(p):
                f, g = os.path.join(tmp, f"out_{r}_{k}.bin"), os.path.join(tmp, f"status_{r}_{k}.txt")
                if os.path.exists(f) and os.path.exists(g):
                    o[r] = np.fromfile(f, dtype=np.uint8)
                    s[r] = tuple(int(v) for v in open(g).read().split())
                    h = os.path.join(tmp, f"out_plain_{r}_{k}.bin")
                    if os.path.exists(h):
                        q[r] = np.fromfile(h, dtype=np.float32)
            outs.append(o)
            stats.append(s)
            plains.append(q)
        return MixedRun(cp.returncode, cp.stderr, outs, stats, plains)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def check_against_model(o, want, run: MixedRun, k, counts, types, what):
    """Call k of `run` against the oracle's Result `o` on the widened inputs and the model's
    vectors `want`: the same outcome class; for every survivor the return code, comm size and
    recoveries, intact guards and inputs, coalesced = the non-empty count, the two movers' HBM
    bytes (4 + the entry's element size per element and launch) and the model's vector."""
    if o.aborted:
        assert run.aborted and not run.outputs[k], (what, run.stderr[-2000:])
        return
    assert not run.aborted, (what, run.stderr[-2000:])
    nonempty = sum(1 for c in counts if c)
    movers = 2 * (4 * sum(counts) + nbytes(counts, types))
    for w, st in enumerate(o.status):
        if st != 0:
            assert w not in run.outputs[k], (what, "rank", w, "died in the oracle")
            continue
        assert w in run.outputs[k], (what, "rank", w, run.stderr[-2000:])
        s = run.status[k][w]
        assert (s[R.RC], s[R.CSIZE], s[R.SIZE_AFTER], s[R.RECOVERIES]) == (o.ret, len(o.order_after), len(o.order_after), o.recoveries), (what, w, s)
        assert s[R.INTACT] == 1, (what, w, "a guard or an input was written")
        assert s[R.COALESCED] == nonempty, (what, w, s)
        assert s[HBM] >= movers, (what, w, s)
        assert same(run.outputs[k][w], want[w], counts, types), (what, "rank", w)
