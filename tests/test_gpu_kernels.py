"""GPU parity of the local-reduce kernel (MPI_Reduce_local) against the CPU oracle.

Bar: bit-exact for every dtype/op on the same inputs (one IEEE op per element for
floats; two's-complement wrap for ints).  Sizes cover empty, ragged, unaligned heads
and tails, non-co-aligned pointers (scalar path) and the full 256 MiB C2 vector.
"""
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NP = {0: np.int32, 1: np.float32, 2: np.int64, 3: np.float64}
UINT = {4: np.uint32, 8: np.uint64}


def _inputs(dt, n, seed, specials=False):
    rng = np.random.default_rng(seed)
    t = NP[dt]
    if np.dtype(t).kind == "f":
        a = (rng.standard_normal(n) * 100).astype(t)
        b = (rng.standard_normal(n) * 100).astype(t)
        if specials and n >= 16:
            sp = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 3.4e38, -3.4e38], dtype=t)
            a[:8] = sp
            b[8:16] = sp
    else:
        info = np.iinfo(t)
        a = rng.integers(info.min, info.max, n, dtype=t, endpoint=True)
        b = rng.integers(info.min, info.max, n, dtype=t, endpoint=True)
    return a, b


def _same_bits(x, y):
    u = UINT[x.dtype.itemsize]
    return np.array_equal(x.view(u), y.view(u))


def _to_dev(a):
    import torch
    return torch.from_numpy(a.copy()).cuda()


@pytest.mark.parametrize("dt", [0, 1, 2, 3])
@pytest.mark.parametrize("op", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 3, 17, 1000, 65537, 1 << 20])
def test_reduce_local_bit_exact(ftar, oracle, dt, op, n):
    import torch
    a, b = _inputs(dt, n, seed=n * 7 + op, specials=(op >= 2 or n > 100))
    x, y = _to_dev(a), _to_dev(b)
    ftar.reduce_local(x, y, op=op)  # y = y <op> x
    torch.cuda.synchronize()
    want = b.copy()
    oracle.reduce_local(a, want, op)
    assert _same_bits(y.cpu().numpy(), want)


@pytest.mark.parametrize("off_in,off_io", [(1, 1), (3, 3), (1, 2), (0, 3), (2, 0)])
def test_reduce_local_unaligned(ftar, oracle, off_in, off_io):
    """Heads/tails (co-aligned offsets) and the scalar path (different alignments)."""
    import torch
    n = 100003
    a, b = _inputs(1, n + 8, seed=11)
    x, y = _to_dev(a), _to_dev(b)
    ftar.reduce_local(x[off_in:off_in + n], y[off_io:off_io + n], count=n, dtype=1, op=0)
    torch.cuda.synchronize()
    want = b.copy()
    part = want[off_io:off_io + n].copy()
    oracle.reduce_local(a[off_in:off_in + n].copy(), part, 0)
    want[off_io:off_io + n] = part
    assert _same_bits(y.cpu().numpy(), want)  # untouched outside the window too


@pytest.mark.parametrize("variant", [0, 1])
def test_reduce_local_c2_full_size(ftar, variant):
    """C2: two 256 MiB float32 vectors; property check against torch's own fp32 add
    (one IEEE add per element, so bit-identical)."""
    import torch
    n = 1 << 26
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(n, device="cuda", generator=g) * 2 - 1
    y = torch.rand(n, device="cuda", generator=g) * 2 - 1
    want = y + x
    ftar.set_reduce_variant(variant)
    try:
        ftar.reduce_local(x, y, op=0)
        torch.cuda.synchronize()
    finally:
        ftar.set_reduce_variant(0)
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("variant,extra", [(0, 4099), (1, 4100)])
def test_reduce_local_beyond_2g_elements(ftar, variant, extra):
    """More than 2^31 elements (8 GiB per vector): 64-bit indexing in both kernels and
    the capped, grid-stride launch; a ragged tail for the register kernel.  Checked
    against torch's fp32 add (one IEEE add per element, so bit-identical)."""
    import torch
    n = (1 << 31) + extra
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.rand(n, device="cuda", generator=g)
    y = torch.rand(n, device="cuda", generator=g)
    want = y + x
    ftar.set_reduce_variant(variant)
    try:
        ftar.reduce_local(x, y, op=0)
        torch.cuda.synchronize()
    finally:
        ftar.set_reduce_variant(0)
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    del x, y, want
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dt", [0, 1, 2, 3])
def test_reduce_local_lds_variant_bit_exact(ftar, oracle, dt):
    import torch
    n = (1 << 20) + 256  # multiple of 16 bytes for every dtype
    a, b = _inputs(dt, n, seed=dt)
    x, y = _to_dev(a), _to_dev(b)
    ftar.set_reduce_variant(1)
    try:
        ftar.reduce_local(x, y, op=0)
        torch.cuda.synchronize()
    finally:
        ftar.set_reduce_variant(0)
    want = b.copy()
    oracle.reduce_local(a, want, 0)
    assert _same_bits(y.cpu().numpy(), want)


def test_reduce_local_rejects_bad_args(ftar):
    import torch
    x = torch.zeros(16, device="cuda")
    with pytest.raises(ftar.FtarError):
        ftar.reduce_local(x, x, dtype=9)


@pytest.mark.parametrize("dt", [0, 2])
@pytest.mark.parametrize("op", [4, 5, 6, 7, 8, 9])
@pytest.mark.parametrize("n", [1, 17, 65537, 1 << 20])
def test_reduce_local_logical_bitwise(ftar, oracle, dt, op, n):
    """MPI's logical / bitwise ops on the integer types: vector body, heads and tails
    bit-exact to the oracle; inputs carry zeros for the logical ops."""
    import torch
    a, b = _inputs(dt, n, seed=n * 3 + op)
    a[::3] = 0
    b[1::5] = 0
    x, y = _to_dev(a), _to_dev(b)
    ftar.reduce_local(x, y, op=op)
    torch.cuda.synchronize()
    want = b.copy()
    oracle.reduce_local(a, want, op)
    assert _same_bits(y.cpu().numpy(), want)


@pytest.mark.parametrize("dt", [1, 3])
def test_reduce_local_bitwise_on_float_refused(ftar, dt):
    """MPI_ERR_OP before any launch; the output is untouched."""
    import torch
    x = torch.ones(1000, device="cuda", dtype=torch.float32 if dt == 1 else torch.float64)
    y = torch.full_like(x, 2.0)
    for op in range(4, 10):
        with pytest.raises(ftar.FtarError, match="code 9"):
            ftar.reduce_local(x, y, op=op)
    torch.cuda.synchronize()
    assert bool((y == 2.0).all())


def _pinned(a):
    import torch
    return torch.from_numpy(a.copy()).pin_memory()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dt", [0, 1, 2, 3])
@pytest.mark.parametrize("op", [0, 2, 3])
@pytest.mark.parametrize("n", [1, 17, 65537, (1 << 20) + 256])
def test_reduce_local_pinned_host(ftar, oracle, variant, dt, op, n):
    """The reference's MPI_Reduce_local works on host buffers: with pinned ones the kernel
    reads and writes them in place over PCIe (zero copy).  Bit-exact to the oracle, both
    kernels, the vector body and the scalar heads / tails."""
    import torch
    a, b = _inputs(dt, n, seed=n * 5 + op + dt, specials=op >= 2)
    x, y = _pinned(a), _pinned(b)
    ftar.set_reduce_variant(variant)
    try:
        ftar.reduce_local(x, y, op=op)
        torch.cuda.synchronize()
    finally:
        ftar.set_reduce_variant(0)
    want = b.copy()
    oracle.reduce_local(a, want, op)
    assert _same_bits(y.numpy(), want)


@pytest.mark.parametrize("where", ["in_host", "inout_host"])
def test_reduce_local_mixed_host_device(ftar, oracle, where):
    """One operand in pinned host memory, the other in HBM."""
    import torch
    n = 300007
    a, b = _inputs(1, n, seed=23)
    x = _pinned(a) if where == "in_host" else _to_dev(a)
    y = _pinned(b) if where == "inout_host" else _to_dev(b)
    ftar.reduce_local(x, y, op=0)
    torch.cuda.synchronize()
    want = b.copy()
    oracle.reduce_local(a, want, 0)
    assert _same_bits(y.cpu().numpy(), want)


@pytest.mark.parametrize("off_in,off_io", [(1, 1), (1, 2)])
def test_reduce_local_pinned_unaligned(ftar, oracle, off_in, off_io):
    import torch
    n = 100003
    a, b = _inputs(1, n + 8, seed=29)
    x, y = _pinned(a), _pinned(b)
    ftar.reduce_local(x[off_in:off_in + n], y[off_io:off_io + n], count=n, dtype=1, op=0)
    torch.cuda.synchronize()
    want = b.copy()
    part = want[off_io:off_io + n].copy()
    oracle.reduce_local(a[off_in:off_in + n].copy(), part, 0)
    want[off_io:off_io + n] = part
    assert _same_bits(y.numpy(), want)


def test_reduce_local_c2_pinned_host_full_size(ftar):
    """C2's two 256 MiB float32 vectors in pinned host memory, reduced in place over PCIe
    (bench.py's e2e.zero_copy); checked against torch's fp32 add on the CPU (one IEEE add
    per element, so bit-identical)."""
    import torch
    n = 1 << 26
    g = torch.Generator().manual_seed(13)
    x = (torch.rand(n, generator=g) * 2 - 1).pin_memory()
    y = (torch.rand(n, generator=g) * 2 - 1).pin_memory()
    want = y + x
    ftar.set_reduce_variant(1)
    try:
        ftar.reduce_local(x, y, op=0)
        torch.cuda.synchronize()
    finally:
        ftar.set_reduce_variant(0)
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))


def test_reduce_local_refuses_pageable_and_overruns(ftar):
    """Pageable host memory (a kernel touching it would fault the GPU) and a range past
    its device allocation are refused with FTAR_ERR_ARG before any launch."""
    import torch
    page = np.arange(4096, dtype=np.float32)
    y = torch.full((4096,), 2.0, device="cuda")
    with pytest.raises(ftar.FtarError, match="code 13"):
        ftar.reduce_local(page.ctypes.data, y, count=4096, dtype=1)
    with pytest.raises(ftar.FtarError, match="code 13"):
        ftar.reduce_local(y, page.ctypes.data, count=4096, dtype=1)
    with pytest.raises(ftar.FtarError):
        ftar.reduce_local(torch.from_numpy(page), y)  # not pinned: refused in the binding
    x = torch.ones(16, device="cuda")
    with pytest.raises(ftar.FtarError, match="code 13"):
        ftar.reduce_local(x, y, count=1 << 30, dtype=1)
    torch.cuda.synchronize()
    assert bool((y == 2.0).all())
    assert np.array_equal(page, np.arange(4096, dtype=np.float32))


def test_short_pinned_buffers_refused(ftar):
    """A pinned host buffer shorter than `count`: refused with FTAR_ERR_ARG by the
    local reduce and by both Allreduce entry points before anything is launched -- the GPU
    would otherwise page-fault past the pinned allocation."""
    import torch
    short = torch.ones(1024).pin_memory()
    y = torch.full((1 << 20,), 2.0).pin_memory()
    yd = torch.full((1 << 20,), 2.0, device="cuda")
    for a, b in ((short, yd), (yd, short), (short, y)):
        with pytest.raises(ftar.FtarError, match="code 13"):
            ftar.reduce_local(a, b, count=1 << 20, dtype=1)
    comm = ftar.Comm.init_rank(f"/ftar-pin-{os.getpid()}", 0, 1, 0)
    try:
        assert comm.allreduce_rabenseifner(short, yd, count=1 << 20) == ftar.ERR_ARG
        assert comm.allreduce_rabenseifner(yd, short, count=1 << 20) == ftar.ERR_ARG
        assert comm.recursive_doubling(short, yd, count=1 << 20) == ftar.ERR_ARG
        assert comm.recursive_doubling(yd, short, count=1 << 20) == ftar.ERR_ARG
        # the same buffers at their own length go through (zero copy on pinned memory)
        assert comm.allreduce_rabenseifner(short, short, count=1024) == 0
    finally:
        comm.finalize()
    torch.cuda.synchronize()
    assert bool((yd == 2.0).all()) and bool((y == 2.0).all()) and bool((short == 1.0).all())


@pytest.mark.timeout(300)
def test_tree_kernels_against_oracle():
    """The mesh's tree kernels on their own (tests/kernel_gpu/tree_check.hip, built by
    __graft_entry__.build()): tree_kernel at p = 2, 4, 8 AND 16 (the schedules reach p = 16
    only with 16 ranks), unroll 1 / 2 / 4, extra destinations (push2), co-aligned and
    mutually misaligned pointers, ragged lengths up to 2^20 + 7, and tree_batch_kernel (the
    one-shot form, 1 / 3 / 8 trees), float32 / float64 / int32 / int64 with SUM, PROD, MAX,
    MIN and MPI's logical / bitwise ops -- bit-exact against the balanced tree computed by
    the oracle's reduce_local, MAX / MIN over NaN, signed zeros and infinities."""
    _run_checker("tree_check")


def _run_checker(name, *args):
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "kernel_gpu", "_build",
                       name)
    assert os.path.exists(exe), "tests/kernel_gpu not built: run __graft_entry__.build()"
    cp = subprocess.run([exe, *args], capture_output=True, text=True, timeout=280)
    assert cp.returncode == 0, (cp.stdout[-3000:], cp.stderr[-2000:])
    assert " 0 failed" in cp.stdout, cp.stdout[-3000:]


@pytest.mark.timeout(300)
def test_segment_kernel_against_oracle():
    """The segment kernel on its own (tests/kernel_gpu/seg_check.hip): 400 random lists of
    up to 16 copy / reduce pieces as the schedules build them -- ragged lengths up to 2^20,
    co-aligned and misaligned pointers, a second destination holding the result or (the
    mid-exchange guard) the local operand's pre-image, grids capped at 2^20 / 1024 / 128 / 7
    workgroups -- bit-exact against the oracle, nothing written outside a destination,
    sources untouched; MAX / MIN over NaN, signed zeros and infinities."""
    _run_checker("seg_check")


def test_tree_kernels_on_half_and_pair_types():
    """tree_check types: tree_kernel and tree_batch_kernel on float16 / bfloat16 (SUM, PROD, MAX,
    MIN) and the three pair types (MAXLOC, MINLOC), which the oracle does not know -- against the
    plain reference of tests/kernel_gpu/ref_types.h (pinned against torch's CPU arithmetic and
    numpy in test_kernel_ref.py, where the inputs are also shown to tell a wrong rounding or
    operand order from the right one).  p = 2, 4, 8 and 16, unroll 1 / 2 / 4, extra destinations,
    both kinds of store, lengths around every boundary of the 2-, 8- and 16-byte elements, heads
    of 7, 5 and 1 elements, 8-byte pairs 4 and 12 bytes past a 16-byte boundary (co-aligned, yet
    the scalar path), mutually misaligned sources; batches of 1 / 3 / 8 trees, capped to 64 / 9
    workgroups.  Bit for bit, NaN-ness where a SUM / PROD expectation is a NaN; guards, sources
    and extra destinations checked."""
    _run_checker("tree_check", "types")


def test_segment_kernel_on_half_and_pair_types():
    """seg_check types: 210 lists of up to 16 copy / reduce pieces at element sizes 2, 8 and 16
    (the same 14 type / op combinations in rotation), windows co-aligned or independent at
    every offset the types' alignment allows, pieces of up to 2 MiB (the interleaved 128 KiB
    prefix, required to occur at every element size), a second destination, grids capped at
    2^20 / 1024 / 128 / 7 workgroups -- against the same reference, every byte outside a
    destination untouched."""
    _run_checker("seg_check", "types")


def test_gather_movers_on_their_own():
    """gather_check: gather_kernel in both directions through launch_gather, with tables and grids
    chosen by the checker (tests/kernel_gpu/gen_movers.h) -- element sizes 1, 2, 4, 8, 16; user buffers
    at every multiple of the type's alignment past a 16-byte boundary (1-byte elements at all 16
    offsets, 2-byte elements at 0 .. 14, 8-byte pairs at 4 and 12, the 16-byte pair at 8), congruent
    to their packed address or not, 1-byte elements behind a packed start of 3 bytes, and 2-byte
    elements against an odd packed address (units of one byte); entries of one element,
    around one vector, of 1023 / 1024 / 1025 bytes, around 4 * 64 and 4 * 256 vectors, one tile
    -1 / 0 / +1 element, an entry ending on a tile edge with another behind it, one entry over five
    tiles, 320 one-element entries in one tile (the deal over the four waves), 1024 entries; user
    buffers in device memory or in pinned host memory; grids of ntiles, min(7, ntiles) and 1 (the
    stride loop).  Expected: concatenation, byte for byte, and every other byte of the arena --
    guards, gaps, the source side -- untouched.  test_kernel_ref.py counts on the CPU that these
    tables reach every unit, path, threshold and tile-edge exit."""
    _run_checker("gather_check")


def test_converting_movers_on_their_own():
    """gather_check cvt: gather_cvt_kernel for float16 and bfloat16 in both directions through
    launch_gather_cvt -- user buffers at every even offset, packed starts giving classes 8, 4, 2
    (with head and tail) and 1, the same sizes in elements and the same three grids, a pinned
    table.  Gather: every 16-bit pattern widened, bit for bit against the reference's decode.
    Scatter at scales 1, 0.5, 1/3, -1, 2^-12, 0 and 3.0000002 against ONE float32 multiplication and
    ONE conversion by the reference (encode16((double)(float)((double)scale * a))): every widened
    pattern, every finite pattern's tie with its neighbour -1 / 0 / +1 ulp of float32, products
    that round in float32 to such a tie, ties in the subnormal range, the overflow edge, -0 and
    products underflowing to -0 (alone and in packed groups), float32-subnormal products,
    infinities and NaNs whose upper 16 bits read as an infinity.  Bit for bit, any NaN where a NaN
    is expected; test_kernel_ref.py shows that a wrong rounding, a fused multiply-convert, a +0 or
    a truncated NaN would each be seen."""
    _run_checker("gather_check", "cvt")


def test_mixed_mover_on_its_own():
    """gather_check mix: gather_mix_kernel in both directions through launch_gather_mix, the type
    words uploaded behind the table as the product lays them out (ftar::mix_types), on the mixed
    tables of gen_movers.h -- the converting sizes (1 .. 257 x 8 elements, one tile -1 / 0 / +1, an
    entry ending on a tile edge, five tiles + 3) with float16, bfloat16 and float32 cycling from
    each of the three, so every size occurs with every type; user buffers at every multiple of the
    entry's own alignment, all congruent (float32 in 16-byte vectors, 2-byte entries of class 8) or
    none (float32 word by word, classes 4, 2, 1); packed starts 0, 4, 8, 12, 20 past a 256-byte
    boundary (float32 heads of 0, 3, 2, 1 words; whole float32 tiles of 1024 and of 1023 vectors);
    320 one-element entries with type periods of 3 (every wave meets every type) and 4 (every wave
    one type); tables of 1024, 1023 and 7 entries (the type array at three offsets); for each of
    the 6 ordered pairs of types a tile edge exactly between them and one 3 elements in front; two
    neighbours of one type; pieces of 1020, 1024 and 1028 packed bytes of every type in one tile;
    pinned tables; the converting tables' pattern, tie and non-finite blocks with float32 entries of
    1, 5 and 4099 elements between them.  Grids of ntiles, min(7, ntiles) and 1.  Gather (launched
    with scale 0.5, which must not be applied): every 16-bit pattern widened, float32 words --
    signalling NaNs among them -- copied bit for bit.  Scatter at the seven scales: a 2-byte entry
    as in `cvt`; a float32 entry (float)((double)scale * a), ONE multiplication, bit for bit on
    +-0, subnormal products, products underflowing to -0, the overflow at 3.0000002, infinities and
    the largest value, any NaN where a NaN is expected.  The whole arena is compared: guards,
    gaps, packed bytes past the total, the source side.  test_kernel_ref.py counts on the CPU that
    these tables reach every (type, wave), neighbour pair, edge, threshold, class, head and loop,
    and that a flushed product, a +0 or an unscaled float32 element would be seen in a word and
    in a vector."""
    _run_checker("gather_check", "mix")


def test_lds_reduce_on_its_own():
    """lds_check: reduce_lds_kernel through launch_reduce_lds with the checker's grid -- all nine
    element types with every op each has, both kinds of store, 1, 63, 64, 255, 256, 257, 1023, 1024,
    1025 and 4 * 1024 + 65 vectors at grids of ntiles, min(3, ntiles) and 1, so that one workgroup
    takes several full tiles and ends in the ragged path.  Inputs with NaN, +-0, infinities and
    pair padding; expected inout = inout op in by the oracle (the four old types) or the plain
    reference, bit for bit (NaN-ness where a SUM / PROD expectation is a NaN); `in` and the guards
    around `inout` untouched."""
    _run_checker("lds_check")
