"""ftar_allreduce_multi jobs under ftrun (test infrastructure): tests/multi/multi_probe.c as the
ranks, against the host-sim build (CPU tests) or libftar.so (GPU tests, every rank on GPU 0).

`run_multi` takes, per call, the counts list and every rank's dense input vector (what the
entries hold, concatenated), and returns per call and rank the dense result, the status tuple
and -- with plain=True -- the result of the plain entry point on the same vector in the same job.
"""
from __future__ import annotations

import fcntl
import glob
import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass

import numpy as np

import harness as H

DIR = os.path.join(H.ROOT, "tests", "multi")
ALL_ON_GPU0 = ",".join(["0"] * 16)
# the issue's lists: sizes around a vector and a 16 KiB tile, an empty entry, then 40 tiny ones
TINY40 = [1 + (i * 5) % 7 for i in range(40)]
COUNTS = [1, 3, 0, 5, 4093, 4099, 2, 2, 2]
# status line of multi_probe.c
RC, CRANK, CSIZE, RECOVERIES, COALESCED, INTACT, KERNELS, PLAIN_RC, SIZE_AFTER = range(9)


def build(gpu: bool = False) -> str:
    """The probe (and what it links against), one build at a time."""
    with open(os.path.join(H.ROOT, "tests", "hostsim", ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not gpu:
            subprocess.run(["make", "-s", "-C", os.path.join(H.ROOT, "tests", "hostsim")], check=True)
        subprocess.run(["make", "-s", "-C", DIR, "gpu" if gpu else "all"], check=True)
    return os.path.join(DIR, "_build", "gpu" if gpu else "", "multi_probe")


@dataclass
class MultiRun:
    returncode: int
    stderr: str
    outputs: list  # [call][rank] -> dense result (bytes viewed as the input dtype)
    status: list   # [call][rank] -> status tuple
    plain: list    # [call][rank] -> the plain entry point's result

    @property
    def aborted(self) -> bool:
        return "MPI_ABORT" in self.stderr


def _semi(v) -> str:
    return ";".join(str(x) for x in v) if isinstance(v, (list, tuple)) else str(v)


def run_multi(algo, calls, p, dtype=0, op=0, kills=(), backend="hostsim", inplace=0, offset=0,
              plain=False, env_extra=None, timeout=120) -> MultiRun:
    """calls: [(counts, [rank r's dense vector])]; dtype and op: one value, or a list with one per
    call.  Vectors of uint8 are raw bytes of any element type."""
    tmp = tempfile.mkdtemp(prefix="ftar_multi_")
    try:
        for k, (counts, ins) in enumerate(calls):
            assert len(ins) == p
            for r, x in enumerate(ins):
                x = np.ascontiguousarray(x)
                assert x.size == sum(counts) or x.dtype == np.uint8
                x.tofile(os.path.join(tmp, f"in_{r}_{k}.bin"))
        gpu = backend == "gpu"
        ftrun = os.path.join(H.PKG if gpu else H.HOSTSIM, "bin", "ftrun")
        probe = os.path.join(DIR, "_build", "gpu" if gpu else "", "multi_probe")
        env = dict(os.environ, FTAR_PROBE_DIR=tmp, FTAR_PROBE_ALGO=algo, FTAR_PROBE_DTYPE=_semi(dtype), FTAR_PROBE_OP=_semi(op),
                   FTAR_MULTI_COUNTS=";".join(",".join(str(c) for c in counts) for counts, _ in calls),
                   FTAR_PROBE_INPLACE=str(inplace), FTAR_PROBE_OFFSET=str(offset), FTAR_MULTI_PLAIN=str(int(plain)),
                   FTAR_HOSTSIM_TAG=os.path.basename(tmp))
        env.pop("FTAR_KILL", None)
        if kills:
            env["FTAR_KILL"] = H.kill_env(kills)
        env.update(env_extra or {})
        cmd = [ftrun, "-np", str(p)] + (["--devmap", ALL_ON_GPU0] if gpu else []) + [probe]
        cp = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
        outs, stats, plains = [], [], []
        for k, (counts, ins) in enumerate(calls):
            o, s, q = {}, {}, {}
            for r in range(p):
                f, g = os.path.join(tmp, f"out_{r}_{k}.bin"), os.path.join(tmp, f"status_{r}_{k}.txt")
                if os.path.exists(f) and os.path.exists(g):
                    o[r] = np.fromfile(f, dtype=ins[0].dtype)
                    s[r] = tuple(int(v) for v in open(g).read().split())
                    h = os.path.join(tmp, f"out_plain_{r}_{k}.bin")
                    if os.path.exists(h):
                        q[r] = np.fromfile(h, dtype=ins[0].dtype)
            outs.append(o)
            stats.append(s)
            plains.append(q)
        return MultiRun(cp.returncode, cp.stderr, outs, stats, plains)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        for f in glob.glob(f"/dev/shm/ftarhs-{os.path.basename(tmp)}-*"):
            try:
                os.unlink(f)
            except OSError:
                pass


def same_bits(a, b) -> bool:
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def same_bits_or_nan(got, want) -> bool:
    """Bit equality, and a NaN (any payload) exactly where `want` holds one."""
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and same_bits(got[~gn], want[~wn])


def check_against_oracle(o, run: MultiRun, k, counts, what, nan_payload=True):
    """Call k of `run` against the oracle's Result on the concatenation: the same outcome class,
    every survivor the oracle's vector bit for bit, return code, comm size and recoveries too.
    nan_payload=False (a float SUM on the GPU against the CPU oracle): a NaN where the oracle
    holds one, of any payload -- include/ftar.h leaves the payload of a computed NaN open, and
    inf + -inf is 0xffc00000 on the oracle's CPU and 0x7fc00000 on the GPU."""
    if o.aborted:
        assert run.aborted and not run.outputs[k], (what, run.stderr[-2000:])
        return
    assert not run.aborted, (what, run.stderr[-2000:])
    nonempty = sum(1 for c in counts if c)
    for w, st in enumerate(o.status):
        if st != 0:
            assert w not in run.outputs[k], (what, "rank", w, "died in the oracle")
            continue
        assert w in run.outputs[k], (what, "rank", w, run.stderr[-2000:])
        s = run.status[k][w]
        assert (s[RC], s[CSIZE], s[SIZE_AFTER], s[RECOVERIES]) == (o.ret, len(o.order_after), len(o.order_after), o.recoveries), (what, w, s)
        assert s[INTACT] == 1, (what, w, "a guard or an input was written")
        assert s[COALESCED] == (nonempty if nonempty > 1 else 0), (what, w, s)
        eq = same_bits if nan_payload else same_bits_or_nan
        assert eq(run.outputs[k][w], o.outputs[w]), (what, "rank", w)
