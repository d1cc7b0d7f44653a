"""Builds and runs the host programs of tests/kernel_plan for the tests that use them
(test_kernel_plan.py, and the element types' own tests at their sizes)."""
import fcntl
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "kernel_plan")


def build_plan_checks():
    os.makedirs(os.path.join(DIR, "_build"), exist_ok=True)
    with open(os.path.join(DIR, "_build", ".lock"), "w") as lk:  # one build at a time (pytest-xdist workers)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", DIR], check=True)


@functools.lru_cache(maxsize=None)  # (two tests ask for esize 2)
def run_planwalk(esize):
    """planwalk_check <esize>, plain and sanitized (a stand-alone program, nothing preloaded):
    both exit 0; the sanitized one really carries the sanitizers.  Returns the number of cases."""
    build_plan_checks()
    plain, san = (os.path.join(DIR, "_build", n) for n in ("planwalk_check", "planwalk_check_san"))
    syms = subprocess.run(["nm", san], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms  # really built with the sanitizers
    counts = []
    for exe in (plain, san):
        cp = subprocess.run([exe, str(esize)], capture_output=True, text=True, timeout=300)
        assert cp.returncode == 0, cp.stdout + cp.stderr[-3000:]
        assert cp.stdout.startswith("OK esize %d " % esize), cp.stdout
        counts.append(int(cp.stdout.split()[3]))
    assert counts[0] == counts[1]
    return counts[0]
