"""ftar_allreduce_multi_acc32 (test infrastructure): the numpy model of the call's definition, and
jobs of tests/acc32/acc32_probe.c under ftrun against libftar.so, every rank on GPU 0.

The model, numpy only.  A vector of 2-byte floats is an array of uint16 bit patterns; `dt` is the
ftar_dtype (16: float16, 17: bfloat16).

    expected = narrow(np.float32(scale) * oracle_fn(widen(inputs), kills, op).outputs[w])

`same` compares two uint16 vectors through their widened values (widening is exact and injective, so
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

import harness as H
import multi_runner as R

DIR = os.path.join(H.ROOT, "tests", "acc32")
F16, BF16 = 16, 17
TYPES = {"float16": F16, "bfloat16": BF16}
# status line of acc32_probe.c: multi_runner's fields, then the call's hbm_bytes
HBM = 9


def widen(u16, dt) -> np.ndarray:
    u16 = np.ascontiguousarray(u16, dtype=np.uint16)
    if dt == F16:
        return u16.view(np.float16).astype(np.float32)
    return (u16.astype(np.uint32) << 16).view(np.float32)


def narrow(f32, dt) -> np.ndarray:
    """One round-to-nearest-even conversion: subnormals kept, overflow to +-inf, NaN -> a quiet NaN."""
    f32 = np.ascontiguousarray(f32, dtype=np.float32)
    if dt == F16:
        with np.errstate(over="ignore", invalid="ignore"):
            return f32.astype(np.float16).view(np.uint16)
    u = f32.view(np.uint32)
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(f32)] = 0x7FC0
    return r


def model(fn, ins16, dt, op, scale, kills=()):
    """(the oracle's Result on the widened inputs, [rank -> expected uint16 vector])."""
    o = fn([widen(x, dt) for x in ins16], list(kills), op=op)
    with np.errstate(over="ignore", invalid="ignore"):
        return o, [narrow(np.float32(scale) * y, dt) for y in o.outputs]


def same(got16, want16, dt) -> bool:
    return R.same_bits_or_nan(widen(got16, dt), widen(want16, dt))


def specials16(oracle, p, n, dt, seed):
    """Random inputs with NaN, +-0 and +-inf: H.with_specials on float32 values, then narrowed, so
    every value is representable."""
    f = H.with_specials(oracle.random_inputs(p, n, seed=seed, dtype=np.float32), seed)
    return [narrow(x, dt) for x in f]


def build() -> str:
    """The probe, one build at a time."""
    with open(os.path.join(H.ROOT, "tests", "hostsim", ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", DIR, "gpu"], check=True)
    return os.path.join(DIR, "_build", "gpu", "acc32_probe")


@dataclass
class Acc32Run:
    returncode: int
    stderr: str
    outputs: list  # [call][rank] -> dense result, uint16
    status: list   # [call][rank] -> status tuple
    plain: list    # [call][rank] -> the plain FLOAT32 entry point's result, float32

    @property
    def aborted(self) -> bool:
        return "MPI_ABORT" in self.stderr


def _one(x) -> str:
    # a scale travels as the hexadecimal form of its float32 value: strtof reads it back exactly
    return float(np.float32(x)).hex() if isinstance(x, (float, np.floating)) else str(x)


def _semi(v) -> str:
    return ";".join(_one(x) for x in v) if isinstance(v, (list, tuple)) else _one(v)


def run_acc32(algo, calls, p, dtype=BF16, op=0, scale=1.0, mode=0, kills=(), inplace=0, offset=0, plain=False,
              env_extra=None, timeout=90) -> Acc32Run:
    """calls: [(counts, [rank r's dense uint16 vector])]; dtype, op, scale and mode: one value, or a
    list with one per call.  plain=True: the probe also runs the plain FLOAT32 entry point on the
    widened vector, which this function supplies as a second input file."""
    tmp = tempfile.mkdtemp(prefix="ftar_acc32_")
    try:
        for k, (counts, ins) in enumerate(calls):
            assert len(ins) == p
            dt = dtype[k] if isinstance(dtype, (list, tuple)) else dtype
            for r, x in enumerate(ins):
                x = np.ascontiguousarray(x)
                assert x.dtype == np.uint16 and x.size == sum(counts)
                x.tofile(os.path.join(tmp, f"in_{r}_{k}.bin"))
                if plain:
                    widen(x, dt).tofile(os.path.join(tmp, f"in32_{r}_{k}.bin"))
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, FTAR_PROBE_ALGO=algo, FTAR_PROBE_DTYPE=_semi(dtype), FTAR_PROBE_OP=_semi(op),
                   FTAR_ACC32_SCALE=_semi([float(x) for x in scale] if isinstance(scale, (list, tuple)) else float(scale)), FTAR_ACC32_MODE=_semi(mode),
                   FTAR_MULTI_COUNTS=";".join(",".join(str(c) for c in counts) for counts, _ in calls),
                   FTAR_PROBE_INPLACE=str(inplace), FTAR_PROBE_OFFSET=str(offset), FTAR_ACC32_PLAIN=str(int(plain)))
        env.pop("FTAR_KILL", None)
        if kills:
            env["FTAR_KILL"] = H.kill_env(kills)
        env.update(env_extra or {})
        cmd = [os.path.join(H.PKG, "bin", "ftrun"), "-np", str(p), "--devmap", R.ALL_ON_GPU0,
               os.path.join(DIR, "_build", "gpu", "acc32_probe")]
        cp = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
        outs, stats, plains = [], [], []
        for k in range(len(calls)):
            o, s, q = {}, {}, {}
            for r in range(p):
                f, g = os.path.join(tmp, f"out_{r}_{k}.bin"), os.path.join(tmp, f"status_{r}_{k}.txt")
                if os.path.exists(f) and os.path.exists(g):
                    o[r] = np.fromfile(f, dtype=np.uint16)
                    s[r] = tuple(int(v) for v in open(g).read().split())
                    h = os.path.join(tmp, f"out_plain_{r}_{k}.bin")
                    if os.path.exists(h):
                        q[r] = np.fromfile(h, dtype=np.float32)
            outs.append(o)
            stats.append(s)
            plains.append(q)
        return Acc32Run(cp.returncode, cp.stderr, outs, stats, plains)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def check_against_model(o, want, run: Acc32Run, k, counts, dt, what):
    """Call k of `run` against the oracle's Result `o` on the widened inputs and the model's
    vectors `want`: the same outcome class; for every survivor the return code, comm size and
    recoveries, intact guards and inputs, coalesced = the non-empty count, 6 bytes of HBM traffic
    per element and launch, and the model's vector."""
    if o.aborted:
        assert run.aborted and not run.outputs[k], (what, run.stderr[-2000:])
        return
    assert not run.aborted, (what, run.stderr[-2000:])
    nonempty, total = sum(1 for c in counts if c), sum(counts)
    for w, st in enumerate(o.status):
        if st != 0:
            assert w not in run.outputs[k], (what, "rank", w, "died in the oracle")
            continue
        assert w in run.outputs[k], (what, "rank", w, run.stderr[-2000:])
        s = run.status[k][w]
        assert (s[R.RC], s[R.CSIZE], s[R.SIZE_AFTER], s[R.RECOVERIES]) == (o.ret, len(o.order_after), len(o.order_after), o.recoveries), (what, w, s)
        assert s[R.INTACT] == 1, (what, w, "a guard or an input was written")
        assert s[R.COALESCED] == nonempty, (what, w, s)
        assert s[HBM] >= 12 * total, (what, w, s)  # the two movers' 6 bytes per element each, plus the schedule's
        assert same(run.outputs[k][w], want[w], dt), (what, "rank", w)
