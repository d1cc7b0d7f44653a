"""TEST helper: the no-fault reduction trees of the two schedules at power-of-two p, restated
in numpy over a pairwise function f(inout, in) -> inout <op> in (MPI_Reduce_local's roles).

Derived from oracle/ftar_oracle.c: test_half_abi.py asserts bit equality with the oracle on
float32; test_gpu_half.py reuses the trees with a pairwise function that rounds to 16 bits at
every combination, which the float32 oracle cannot express.
"""
import numpy as np


def raben_tree(xs, f):
    """Rabenseifner, p a power of two (no pre-step): recursive halving -- at step s a rank
    keeps the lower half of its window (wsize / 2 elements) if its rank is below its partner's
    (rank ^ 2^s), else the upper one, and reduces rbuf = rbuf <op> partner's there
    (ftar_oracle.c: rb_window and the reduce-scatter loop); the allgather then copies every
    final block to everyone.  Returns the one vector all ranks end with."""
    p, n = len(xs), xs[0].size
    buf = [np.array(x, copy=True) for x in xs]
    lo, size = [0] * p, [n] * p
    mask = 1
    while mask < p:
        new = [b.copy() for b in buf]
        for r in range(p):
            d = r ^ mask
            half = size[r] // 2
            a, m = (lo[r], half) if r < d else (lo[r] + half, size[r] - half)
            new[r][a:a + m] = f(buf[r][a:a + m], buf[d][a:a + m])
            lo[r], size[r] = a, m
        buf = new
        mask <<= 1
    out = np.empty_like(buf[0])
    for r in range(p):
        out[lo[r]:lo[r] + size[r]] = buf[r][lo[r]:lo[r] + size[r]]
    return out


def rd_tree(xs, f):
    """Recursive doubling, p a power of two: at distance d a rank combines its accumulator
    with rank ^ d's -- src = src <op> received, except at the last step, where the result is
    formed in dst: dst = received <op> src (ftar_oracle.c: the distance loop).  Returns every
    rank's result."""
    p = len(xs)
    acc = [np.array(x, copy=True) for x in xs]
    d = 1
    while d < p:
        last = 2 * d >= p
        acc = [f(acc[r ^ d], acc[r]) if last else f(acc[r], acc[r ^ d]) for r in range(p)]
        d *= 2
    return acc
