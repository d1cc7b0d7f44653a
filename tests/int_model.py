"""TEST model of the 8-, 16-bit and unsigned integer types (FTAR_INT8 = 48 .. FTAR_UINT64 = 53),
shared by the CPU tests (test_int_abi.py, test_int_ref.py) and the GPU tests (test_gpu_int.py).

* `combine(op)`: include/ftar.h's rule as numpy on the element's own dtype, x = inout, y = in:
  SUM / PROD wrap modulo 2^w (numpy's fixed-width integer arithmetic, overflow warnings off),
  MAX / MIN `(x > y) ? x : y` in the dtype's own signedness, logical ops 0 / 1, bitwise ops on
  the bits.
* operand sets: every 8-bit pair; every 16-bit pattern against 48 partners (the rule of
  test_kernel_ref.py: 16 specials as `in`, the same as `inout`, 16 rotations); specials and random
  values for the 32- and 64-bit unsigned types.
* the value maps of the kill tests: the unchanged oracle knows int64, so a schedule on a narrow or
  unsigned type is checked against the oracle's int64 run on MAPPED values, and the oracle's
  result is mapped back.  `to_oracle` / `from_oracle` and why each is exact are below.
"""
import numpy as np

INT8, UINT8, INT16, UINT16, UINT32, UINT64 = 48, 49, 50, 51, 52, 53
NP = {INT8: np.int8, UINT8: np.uint8, INT16: np.int16, UINT16: np.uint16, UINT32: np.uint32, UINT64: np.uint64}
NAMES = {INT8: "int8", UINT8: "uint8", INT16: "int16", UINT16: "uint16", UINT32: "uint32", UINT64: "uint64"}
TYPES = tuple(NP)
SUM, PROD, MAX, MIN, LAND, BAND, LOR, BOR, LXOR, BXOR = range(10)
OPS = tuple(range(10))
OP_NAMES = ("sum", "prod", "max", "min", "land", "band", "lor", "bor", "lxor", "bxor")


def combine(op):
    """inout <op> in on arrays of one integer dtype; the result has that dtype."""
    def f(x, y):
        assert x.dtype == y.dtype and x.dtype.kind in "iu"
        t = x.dtype
        with np.errstate(over="ignore"):
            if op == SUM:
                return (x + y).astype(t)
            if op == PROD:
                return (x * y).astype(t)
        if op == MAX:
            return np.where(x > y, x, y)
        if op == MIN:
            return np.where(x < y, x, y)
        if op == LAND:
            return ((x != 0) & (y != 0)).astype(t)
        if op == LOR:
            return ((x != 0) | (y != 0)).astype(t)
        if op == LXOR:
            return ((x != 0) != (y != 0)).astype(t)
        return {BAND: x & y, BOR: x | y, BXOR: x ^ y}[op]
    return f


def reduce_ranks(ins, op):
    """The Allreduce of the ranks' vectors: every op is exactly associative and commutative on
    these types, so any order gives the bits of every schedule."""
    out = ins[0].copy()
    for x in ins[1:]:
        out = combine(op)(out, x)
    return out


def specials(dt):
    """Around 0, 2^(w-1) and 2^w - 1, as the dtype's own values."""
    w = 8 * np.dtype(NP[dt]).itemsize
    top, full = 1 << (w - 1), (1 << w) - 1
    u = np.array([0, 1, 2, 3, top - 2, top - 1, top, top + 1, full - 1, full, 0x10, 0x0F, full >> 4, 0x55, 0xAA & full, top >> 1],
                 dtype=np.uint64)
    return u.astype({8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}[w]).view(NP[dt])


def operands(dt, seed=5):
    """(inout, in) for the reference and the local-reduce tests."""
    t = NP[dt]
    w = 8 * np.dtype(t).itemsize
    if w == 8:  # every pair
        pat = np.arange(256, dtype=np.uint8)
        return np.repeat(pat, 256).view(t), np.tile(pat, 256).view(t)
    sp = specials(dt)
    assert sp.size == 16
    if w == 16:  # every pattern against 48 partners
        pat = np.arange(1 << 16, dtype=np.uint16).view(t)
        xs, ys = [], []
        for s in sp:
            const = np.full(pat.size, s, dtype=t)
            xs += [pat, const]
            ys += [const, pat]
        for k in range(16):
            xs.append(pat)
            ys.append(np.roll(pat, 4099 * (k + 1) + (1 << 11) * k))
        return np.concatenate(xs), np.concatenate(ys)
    rng = np.random.default_rng(seed + dt)
    rnd = rng.integers(0, 1 << w, size=(2, 8192), dtype=np.uint64 if w == 64 else np.uint32, endpoint=False).astype(t)
    x = np.concatenate([np.repeat(sp, 16), rnd[0], np.resize(sp, 4096)])
    y = np.concatenate([np.tile(sp, 16), rnd[1], rng.integers(0, 1 << w, size=4096, dtype=np.uint64).astype(t)])
    return x, y


# ---- the oracle's int64 on mapped values ---------------------------------------------------
# For a w-bit type T and u in T (as a Python / int64 value after sign- or zero-extension, e(u)):
#   SUM, PROD      e is a ring homomorphism modulo 2^w: the int64 result (itself modulo 2^64, and
#                  2^w divides 2^64), taken modulo 2^w, is T's.  Exact for any inputs; the kill
#                  tests choose PROD inputs whose exact product fits int64 but not w bits, so the
#                  truncation is exercised and the oracle's own arithmetic never wraps.
#   BAND, BOR,     bitwise on the extension and truncated: the low w bits of the extension are u's.
#   BXOR
#   LAND, LOR,     e(u) != 0 exactly when u != 0.
#   LXOR
#   MAX, MIN       e preserves T's order for every type but uint64, whose values above 2^63 do not
#                  fit; there u ^ 2^63 read as int64 preserves the order (it subtracts 2^63), and
#                  MAX / MIN return one of their operands, so mapping back is the same xor.
def to_oracle(a, dt, op):
    if dt == UINT64:
        if op in (MAX, MIN):
            return (a ^ np.uint64(1 << 63)).view(np.int64)
        return a.view(np.int64)  # two's complement: the same ring modulo 2^64, the same bits
    return a.astype(np.int64)


def from_oracle(r, dt, op):
    if dt == UINT64:
        if op in (MAX, MIN):
            return r.view(np.uint64) ^ np.uint64(1 << 63)
        return r.view(np.uint64).copy()
    w = 8 * np.dtype(NP[dt]).itemsize
    low = (r.view(np.uint64) & np.uint64((1 << w) - 1))
    return low.astype({8: np.uint8, 16: np.uint16, 32: np.uint32}[w]).view(NP[dt])


def int64_combine(op):
    """The oracle's int64 rule (MPI_Reduce_local on MPI_INT64_T) as numpy: what `to_oracle` /
    `from_oracle` must commute with.  It is `combine` itself applied to int64 arrays -- numpy's int64
    arithmetic stands in for the oracle's C, which tests/test_oracle.py pins."""
    return combine(op)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)
