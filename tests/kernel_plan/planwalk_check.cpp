// planwalk_check.cpp -- TEST: host-side coverage check of the work plans at one element size.
//
//   planwalk_check 1|2|4|8|16
//
// For windows at every byte offset 0..15 the type's alignment allows (1, 2, 4 bytes for the
// integers and floats of that size, 4 for the 8-byte types -- MPI's FLOAT_INT and 2INT are pairs of
// 4-byte fields -- and 8 for the 16-byte DOUBLE_INT), a last source that shares the offset or not,
// and sizes from nothing to several tiles, this program runs ftar::plan_segments, ftar::plan_tree,
// ftar::plan_tree_batch and ftar::cap_tree_batch (ftar_plan.cpp) and replays the kernels' own index
// arithmetic (map_block / vec_body / scalar_body, tree_body) on the host, counting how often every
// element is written: exactly once, no operand misaligned to the type, vector accesses 16-byte
// aligned on every operand and inside the window, heads and tails shorter than a vector, and a
// vector body exactly where check_body() says.  What the element sizes bring: heads of up to 15
// elements and windows on odd byte addresses (1), Raben's blocks on odd element offsets (2), 8-byte
// elements in buffers that are only 4-byte aligned (8), one element per vector, so no head or tail
// can be split off and a window at 8 mod 16 has no vector body at all (16).  No GPU needed; built
// plain and, together with the planners, under ASan + UBSan (Makefile).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../fault-tolerant_amd/csrc/ftar_kernels.h"

using namespace ftar;

static size_t ES, EPV; // element size, elements per 16-byte vector
static unsigned ALIGN; // the alignment of the type's C layout: the step of the byte offsets

// Every count some element size needs: 0..64 are added in main (every head and tail length at 1
// and 2 bytes), as is one element count past a full 16 KiB tile.
static const size_t kSizes[] = {255, 256, 257, 1031, 2048 + 5, 3 * 1024 + 5, 3 * 2048 + 5, 8192, 8192 + 7, 16397,
                                3 * 8192 + 40, 65541, 300000};

// mo: byte offset mod 16 of the output and of every operand but one; mx: of that one
static int fail(const char *what, size_t n, unsigned mo, unsigned mx)
{
    fprintf(stderr, "esize %zu, n %zu, out at byte %u, source at byte %u: %s\n", ES, n, mo, mx, what);
    return 1;
}

// THE co-alignment rule: a vector body needs every operand at the output's offset mod 16 and that
// offset on an element boundary (an 8-byte element at 4 mod 8 never reaches a 16-byte boundary)
static bool coaligned(unsigned mo, unsigned mx) { return mo == mx && mo % ES == 0; }
// ... and then two vectors' worth of elements always hold a whole aligned one
static int check_body(bool has_body, const char *plan, size_t n, unsigned mo, unsigned mx)
{
    const bool co = coaligned(mo, mx);
    if (co ? has_body || n < 2 * EPV : !has_body) return 0;
    char what[96];
    snprintf(what, sizeof(what), "%s: %s", plan,
             co ? "co-aligned operands without a vector body" : "a vector body on operands that are not co-aligned");
    return fail(what, n, mo, mx);
}

// one element written once more; false if outside [0, n)
static bool hit(std::vector<uint8_t> &cnt, size_t e)
{
    if (e >= cnt.size()) return false;
    cnt[e]++;
    return true;
}
static bool once(const std::vector<uint8_t> &cnt)
{
    for (uint8_t c : cnt)
        if (c != 1) return false;
    return true;
}

static int check_segments(size_t n, unsigned mo, unsigned mx, unsigned max_blocks, int kind, bool with_out2)
{
    const uintptr_t base = (uintptr_t)1 << 40;
    SegIn in;
    in.kind = kind;
    in.out = (void *)(base + mo);
    in.x = (const void *)(base + ((uintptr_t)1 << 36) + mx);
    in.y = (const void *)(base + ((uintptr_t)2 << 36) + mo);
    in.n = n;
    in.out2 = with_out2 ? (void *)(base + ((uintptr_t)3 << 36) + mo) : nullptr;
    KSegList L;
    const unsigned grid = plan_segments(&in, 1, ES, max_blocks, &L);
    if (n == 0) return grid == 0 ? 0 : fail("segments: a grid for nothing", n, mo, mx);
    if (grid == 0) return fail("segments: no grid", n, mo, mx);
    std::vector<uint8_t> cnt(n, 0);
    bool any_vec = false;
    for (unsigned b = 0; b < grid; b++) {
        const BlockWork w = map_block(L, b);
        if (w.seg < 0 || w.seg >= L.nseg || w.stride == 0) return fail("segments: bad block map", n, mo, mx);
        const KSeg &S = L.s[w.seg];
        const intptr_t off = (intptr_t)S.out - (intptr_t)in.out;
        if (off < 0 || off % (intptr_t)ES || (intptr_t)S.x - (intptr_t)in.x != off)
            return fail("segments: piece offsets", n, mo, mx);
        const uintptr_t all = (uintptr_t)S.out | (uintptr_t)S.x | (uintptr_t)S.y | (uintptr_t)S.out2;
        if (all % ALIGN) return fail("segments: an access misaligned to the type", n, mo, mx);
        const size_t e0 = (size_t)off / ES;
        if (S.vec) { // vec_body: tiles w.first, w.first + w.stride, ... of kTileVecs vectors
            any_vec = true;
            if ((all & 15) || S.n % EPV) return fail("segments: vector piece not 16-byte aligned", n, mo, mx);
            const size_t nv = S.n / EPV;
            for (size_t t = w.first; t * kTileVecs < nv; t += w.stride)
                for (size_t v = t * kTileVecs; v < nv && v < (t + 1) * kTileVecs; v++)
                    for (size_t k = 0; k < EPV; k++)
                        if (!hit(cnt, e0 + v * EPV + k)) return fail("segments: vector past the end", n, mo, mx);
        } else { // scalar_body: kBlock elements per block slot
            if (S.n >= 2 * EPV && coaligned(mo, mx)) return fail("segments: a scalar piece of a vector's length and more", n, mo, mx);
            for (size_t s = w.first; s * kBlock < S.n; s += w.stride)
                for (size_t i = s * kBlock; i < S.n && i < (s + 1) * kBlock; i++)
                    if (!hit(cnt, e0 + i)) return fail("segments: element past the end", n, mo, mx);
        }
    }
    if (!once(cnt)) return fail("segments: an element not written exactly once", n, mo, mx);
    return check_body(any_vec, "segments", n, mo, mx);
}

// tree_body's index arithmetic for one tree: workgroups [0, nblocks)
static int walk_tree(const TreeArgs &A, int p, unsigned nblocks, size_t n, unsigned mo, unsigned mx)
{
    const unsigned U = A.unroll;
    std::vector<uint8_t> cnt(n, 0);
    for (int j = 0; j < p; j++)
        if ((uintptr_t)A.src[j] % ALIGN) return fail("tree: a source misaligned to the type", n, mo, mx);
    if (A.nv) {
        if (A.nvb == 0) return fail("tree: a vector body without workgroups", n, mo, mx);
        for (int j = 0; j < p; j++)
            if (((uintptr_t)A.src[j] + A.head * ES) & 15) return fail("tree: source vectors misaligned", n, mo, mx);
        if (((uintptr_t)A.out + A.head * ES) & 15) return fail("tree: output vectors misaligned", n, mo, mx);
        for (int o = 0; o < A.nmore; o++)
            if (((uintptr_t)A.more[o] + A.head * ES) & 15) return fail("tree: pushed vectors misaligned", n, mo, mx);
    }
    if (A.head >= EPV || A.head + A.nv * EPV > n) return fail("tree: head / body outside the window", n, mo, mx);
    if (A.nv && n - (A.head + A.nv * EPV) >= EPV) return fail("tree: a tail of a whole vector", n, mo, mx);
    for (unsigned b = 0; b < nblocks; b++) {
        if (b < A.nvb) {
            for (size_t c = b; c * kBlock * U < A.nv; c += A.nvb)
                for (unsigned t = 0; t < (unsigned)kBlock; t++)
                    for (unsigned u = 0; u < U; u++) {
                        const size_t i = c * kBlock * U + t + (size_t)u * kBlock;
                        if (i >= A.nv) continue;
                        for (size_t k = 0; k < EPV; k++)
                            if (!hit(cnt, A.head + i * EPV + k)) return fail("tree: vector past the end", n, mo, mx);
                    }
            continue;
        }
        const size_t tail0 = A.head + A.nv * EPV, nscalar = A.head + (A.n - tail0);
        const size_t stride = (size_t)(nblocks - A.nvb) * kBlock;
        for (unsigned t = 0; t < (unsigned)kBlock; t++)
            for (size_t k = (size_t)(b - A.nvb) * kBlock + t; k < nscalar; k += stride)
                if (!hit(cnt, k < A.head ? k : tail0 + (k - A.head))) return fail("tree: element past the end", n, mo, mx);
    }
    if (!once(cnt)) return fail("tree: an element not written exactly once", n, mo, mx);
    return check_body(A.nv != 0, "tree", n, mo, mx);
}

static void fill_tree(TreeArgs *A, int p, size_t n, unsigned mo, unsigned mx, unsigned unroll, int nmore, int slot)
{
    const uintptr_t base = (uintptr_t)(slot + 1) << 44;
    *A = TreeArgs{};
    // source 0 is the rank's own window (aligned like the output), the last one the odd one out
    for (int j = 0; j < p; j++) A->src[j] = (const void *)(base + ((uintptr_t)(j + 1) << 36) + (j == p - 1 ? mx : mo));
    A->out = (void *)(base + mo);
    A->nmore = nmore;
    for (int o = 0; o < nmore; o++) A->more[o] = (void *)(base + ((uintptr_t)(20 + o) << 36) + mo);
    A->n = n;
    A->unroll = unroll;
}

static int check_tree(int p, size_t n, unsigned mo, unsigned mx, unsigned unroll, int nmore)
{
    TreeArgs A;
    fill_tree(&A, p, n, mo, mx, unroll, nmore, 0);
    const unsigned grid = plan_tree(&A, p, ES, 262144);
    if (n == 0) return 0; // the schedules launch no tree over nothing
    if (grid == 0) return fail("tree: no grid", n, mo, mx);
    if (A.unroll != 1 && !(p == 4 || p == 8)) return fail("tree: unrolled where no kernel is", n, mo, mx);
    return walk_tree(A, p, grid, n, mo, mx);
}

// the one-shot form: p trees over consecutive windows of one vector (Raben's blocks, which fall on
// odd element offsets and, at 1-byte elements, odd byte addresses), then the same batch capped to
// few workgroups
static int check_batch(int p, size_t n, unsigned mo, unsigned mx, unsigned cap)
{
    TreeBatch B;
    B.nt = 0;
    B.sig = KSignal{};
    std::vector<size_t> len;
    std::vector<unsigned> tmo, tmx;
    size_t at = 0;
    for (int k = 0; k < p; k++) { // near-equal blocks; an empty one gets no tree (build_batch)
        const size_t m = n / p + ((size_t)k < n % p);
        if (m == 0) continue;
        len.push_back(m);
        tmo.push_back((unsigned)((mo + at * ES) % 16));
        tmx.push_back((unsigned)((mx + at * ES) % 16));
        fill_tree(&B.t[B.nt], p, m, tmo.back(), tmx.back(), 1, 0, k);
        B.nt++;
        at += m;
    }
    if (B.nt == 0) return 0;
    unsigned grid = plan_tree_batch(&B, p, ES, 262144);
    if (grid == 0 || grid != B.first[B.nt]) return fail("batch: grid", n, mo, mx);
    if (cap) {
        const unsigned g = cap_tree_batch(&B, cap);
        if (g) {
            if (g > cap || g != B.first[B.nt]) return fail("batch: capped grid", n, mo, mx);
            grid = g;
        }
    }
    for (int k = 0; k < B.nt; k++) {
        if (B.first[k + 1] <= B.first[k]) return fail("batch: workgroup ranges", n, mo, mx);
        if (walk_tree(B.t[k], p, B.first[k + 1] - B.first[k], len[k], tmo[k], tmx[k])) return 1;
    }
    return 0;
}

// Operands that share no offset are all scalar, whatever the pair: every pair at the small sizes,
// a few at the large ones.  Only the 1- and 2-byte elements have pairs enough to need it.
static bool walked(size_t n, unsigned mo, unsigned mx)
{
    if (mo == mx || ES > 2 || n <= 64 || (mo + mx) % 5 == 0) return true;
    return ES == 2 && (n <= 20000 || (mo / 2 + mx / 2) % 3 == 0);
}

int main(int argc, char **argv)
{
    ES = argc == 2 ? (size_t)atoi(argv[1]) : 0;
    if (ES != 1 && ES != 2 && ES != 4 && ES != 8 && ES != 16) {
        fprintf(stderr, "usage: planwalk_check 1|2|4|8|16\n");
        return 2;
    }
    EPV = 16 / ES;
    ALIGN = ES == 8 ? 4 : ES == 16 ? 8 : (unsigned)ES;
    std::vector<size_t> sizes;
    for (size_t n = 0; n <= 64; n++) sizes.push_back(n);
    sizes.insert(sizes.end(), kSizes, kSizes + sizeof(kSizes) / sizeof(kSizes[0]));
    sizes.push_back((kTileBytes + 16) / ES + 3);
    long cases = 0;
    for (size_t n : sizes)
        for (unsigned mo = 0; mo < 16; mo += ALIGN)
            for (unsigned mx = 0; mx < 16; mx += ALIGN) {
                if (!walked(n, mo, mx)) continue;
                for (int kind : {kReduce, kCopy}) {
                    if (check_segments(n, mo, mx, 262144, kind, kind == kCopy)) return 1;
                    if (check_segments(n, mo, mx, 3, kind, false)) return 1; // capped grid: blocks loop
                    cases += 2;
                }
                for (int p : {2, 4, 8, 16})
                    for (unsigned u : {1u, 2u, 4u}) {
                        if (check_tree(p, n, mo, mx, u, (p <= 8 && u == 1) ? p - 1 : 0)) return 1;
                        cases++;
                    }
                for (int p : {2, 4, 8}) {
                    if (check_batch(p, n, mo, mx, 0) || check_batch(p, n, mo, mx, 4 * (unsigned)p)) return 1;
                    cases += 2;
                }
            }
    printf("OK esize %zu %ld cases\n", ES, cases);
    return 0;
}
