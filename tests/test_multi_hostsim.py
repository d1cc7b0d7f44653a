"""ftar_allreduce_multi as real processes on the host-sim build (no GPU): tests/multi/multi_probe.c
under ftrun, every entry in a buffer of its own.  The call must be exactly the plain schedule on
the dense concatenation of the entries: every rank's result equals, bit for bit, the unchanged
oracle on np.concatenate(inputs) -- without kills at p = 2, 3, 4, 5 for both schedules, and with
the kills the existing suites use, where the oracle decides between recovery and abort and the
job must end the same way.  (The host-sim device layer has no gather kernel: the shared host C
moves the entries with FDEV_COPY segments in groups of FDEV_MAX_SEGS, the fallback this file
exercises; the kernel is tests/test_gpu_multi.py's.)"""
import numpy as np
import pytest

import harness as H
import multi_runner as R

LISTS = {"mixed": R.COUNTS, "tiny40": R.TINY40}


@pytest.fixture(scope="module")
def probe(hostsim):
    return R.build()


def _fn(oracle, algo):
    return oracle.rabenseifner if algo == "raben" else oracle.recursive_doubling


def _inputs(oracle, p, n, case, seed):
    if case == "int32_sum":
        return oracle.random_inputs(p, n, seed=seed, dtype=np.int32), 0, 0
    ins = H.with_specials(oracle.random_inputs(p, n, seed=seed, dtype=np.float32), seed)
    return ins, 1, 0 if case == "float32_sum" else 2


@pytest.mark.parametrize("case", ["int32_sum", "float32_sum", "float32_max"])
@pytest.mark.parametrize("p", [2, 3, 4, 5])
@pytest.mark.parametrize("algo", ["raben", "rd"])
def test_nofault_equals_the_oracle_on_the_concatenation(probe, oracle, algo, p, case):
    """Both lists as two calls of one job, out of place; then in place with every buffer one
    element past a 16-byte boundary."""
    calls, wants = [], []
    for k, (name, counts) in enumerate(LISTS.items()):
        ins, dt, op = _inputs(oracle, p, sum(counts), case, seed=100 * p + k)
        calls.append((counts, ins))
        wants.append(_fn(oracle, algo)(ins, op=op))
    for inplace, offset in ((0, 0), (1, 1)):
        r = R.run_multi(algo, calls, p, dtype=dt, op=op, inplace=inplace, offset=offset)
        assert r.returncode == 0, r.stderr[-2000:]
        for k, (counts, _) in enumerate(calls):
            R.check_against_oracle(wants[k], r, k, counts, (algo, p, case, k, inplace))


KILLS = [("raben", 5, (4, 1, 1, 1)), ("raben", 5, (3, 2, 0, 1)), ("rd", 6, (1, 1, 1, 2)), ("rd", 6, (3, 1, 1, 3))]


@pytest.mark.parametrize("algo,p,kill", KILLS, ids=[f"{a}-p{p}-{'_'.join(map(str, k))}" for a, p, k in KILLS])
def test_kills_end_as_the_oracle_says(probe, oracle, algo, p, kill):
    for case in ("int32_sum", "float32_max"):
        ins, dt, op = _inputs(oracle, p, sum(R.COUNTS), case, seed=7 * p)
        o = _fn(oracle, algo)(ins, [kill], op=op)
        r = R.run_multi(algo, [(R.COUNTS, ins)], p, dtype=dt, op=op, kills=[kill])
        R.check_against_oracle(o, r, 0, R.COUNTS, (algo, p, kill, case))
        assert o.aborted or o.status[kill[0]] != 0, "the kill point was not reached"


def test_multi_equals_the_plain_entry_point_in_the_same_job(probe, oracle):
    """... and a call sequence whose totals grow, shrink and grow again (the staging regrows)."""
    p = 3
    lists = [R.TINY40, R.COUNTS, [2, 2], R.COUNTS + [9000, 1]]
    calls = [(c, H.with_specials(oracle.random_inputs(p, sum(c), seed=k, dtype=np.float32), k)) for k, c in enumerate(lists)]
    r = R.run_multi("raben", calls, p, dtype=1, op=2, plain=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for k, (counts, ins) in enumerate(calls):
        R.check_against_oracle(oracle.rabenseifner(ins, op=2), r, k, counts, ("sequence", k))
        for w in range(p):
            assert r.status[k][w][R.PLAIN_RC] == 0
            assert R.same_bits(r.outputs[k][w], r.plain[k][w]), (k, w)
