"""Host-side coverage checks of the work plans (tests/kernel_plan): the grid planners
(fault-tolerant_amd/csrc/ftar_plan.cpp) and the block -> (piece, tile) map the kernel itself calls
process every vector tile and scalar element of every segment exactly once -- interleaved, capped
and misaligned launches included.  Plain host programs (g++), run on the CPU; the walker also as
a build whose checker and planners are both under ASan + UBSan."""
import os
import subprocess

from plan_checks import DIR, build_plan_checks, run_planwalk


def test_plan_covers_every_unit_once():
    build_plan_checks()
    cp = subprocess.run([os.path.join(DIR, "_build", "plan_check"), "5000"],
                        capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout.startswith("OK 5000 cases")


def test_planners_are_under_the_sanitizers():
    """The sanitized walker links its own sanitized build of the planners, not a product object."""
    build_plan_checks()
    syms = subprocess.run(["nm", "-C", os.path.join(DIR, "_build", "ftar_plan_san.o")], capture_output=True, text=True,
                          check=True).stdout
    for fn in ("plan_segments", "plan_tree", "plan_tree_batch", "cap_tree_batch"):
        assert " T ftar::%s(" % fn in syms, fn
    assert "__asan_" in syms and "__ubsan_handle" in syms


def test_plans_cover_four_byte_elements():
    """plan_segments, plan_tree, plan_tree_batch and cap_tree_batch at esize 4, the benchmark's
    own: (65 + 13 + 1) sizes x 4 x 4 byte offsets x 22 plans."""
    assert run_planwalk(4) >= 79 * 16 * 22
