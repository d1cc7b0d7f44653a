// planpair_check.cpp -- TEST: host-side coverage check of the work plans at the pair types'
// element sizes, 8 and 16 bytes.
//
// The pair types bring the first 16-byte element (one element per vector: no head or tail can
// be split off it, and a window at 8 mod 16 has no vector body at all) and 8-byte elements whose
// buffers are only 4-byte aligned.  For both sizes, windows at every misalignment the type's
// alignment allows (multiples of 4 bytes at 8, of 8 bytes at 16), sources that share it or not,
// and the counts of the GPU test, this program runs ftar::plan_segments, ftar::plan_tree and
// ftar::plan_tree_batch and replays the kernels' own index arithmetic (map_block / vec_body /
// scalar_body, tree_body) on the host, counting how often every element is written: exactly
// once, vector accesses 16-byte aligned on every operand and inside the window, a vector body
// exactly where the operands are co-aligned on a multiple of the element size.  No GPU needed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../fault-tolerant_amd/csrc/ftar_kernels.h"

using namespace ftar;

static size_t ES = 8, EPV = 2; // element size, elements per 16-byte vector
static const size_t kSizes[] = {0, 1, 2, 3, 5, 255, 256, 257, 1031, 2048 + 5, 16397, 3 * 1024 + 5, 3 * 2048 + 5, 65541, 300000};

static int fail(const char *what, size_t n, unsigned mo, unsigned mx)
{
    fprintf(stderr, "esize %zu, n %zu, out at byte %u, source at byte %u: %s\n", ES, n, mo, mx, what);
    return 1;
}

// one element written once more; false if outside [0, n)
static bool hit(std::vector<uint8_t> &cnt, size_t e)
{
    if (e >= cnt.size()) return false;
    cnt[e]++;
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
        const size_t e0 = (size_t)off / ES;
        if (S.vec) { // vec_body: tiles w.first, w.first + w.stride, ... of kTileVecs vectors
            any_vec = true;
            if ((((uintptr_t)S.out | (uintptr_t)S.x | (uintptr_t)S.y | (uintptr_t)S.out2) & 15) || S.n % EPV)
                return fail("segments: vector piece not 16-byte aligned", n, mo, mx);
            const size_t nv = S.n / EPV;
            for (size_t t = w.first; t * kTileVecs < nv; t += w.stride)
                for (size_t v = t * kTileVecs; v < nv && v < (t + 1) * kTileVecs; v++)
                    for (size_t k = 0; k < EPV; k++)
                        if (!hit(cnt, e0 + v * EPV + k)) return fail("segments: vector past the end", n, mo, mx);
        } else { // scalar_body: 256 elements per block slot
            for (size_t s = w.first; s * 256 < S.n; s += w.stride)
                for (size_t i = s * 256; i < S.n && i < (s + 1) * 256; i++)
                    if (!hit(cnt, e0 + i)) return fail("segments: element past the end", n, mo, mx);
        }
    }
    for (size_t e = 0; e < n; e++)
        if (cnt[e] != 1) return fail(cnt[e] ? "segments: element written twice" : "segments: element never written", n, mo, mx);
    if (mo == mx && mo % ES == 0 && n >= 2 * EPV && !any_vec) return fail("segments: co-aligned operands without a vector body", n, mo, mx);
    if ((mo != mx || mo % ES) && any_vec) return fail("segments: a vector body on operands that are not co-aligned on the element size", n, mo, mx);
    return 0;
}

// tree_body's index arithmetic for one tree: workgroups [0, nblocks)
static int walk_tree(const TreeArgs &A, int p, unsigned nblocks, size_t n, unsigned mo, unsigned mx)
{
    const unsigned U = A.unroll;
    std::vector<uint8_t> cnt(n, 0);
    if (A.nv) {
        if (A.nvb == 0) return fail("tree: a vector body without workgroups", n, mo, mx);
        for (int j = 0; j < p; j++)
            if (((uintptr_t)A.src[j] + A.head * ES) & 15) return fail("tree: source vectors misaligned", n, mo, mx);
        if (((uintptr_t)A.out + A.head * ES) & 15) return fail("tree: output vectors misaligned", n, mo, mx);
        for (int o = 0; o < A.nmore; o++)
            if (((uintptr_t)A.more[o] + A.head * ES) & 15) return fail("tree: pushed vectors misaligned", n, mo, mx);
    }
    if (A.head >= EPV || A.head + A.nv * EPV > n) return fail("tree: head / body outside the window", n, mo, mx);
    for (unsigned b = 0; b < nblocks; b++) {
        if (b < A.nvb) {
            for (size_t c = b; c * 256 * U < A.nv; c += A.nvb)
                for (unsigned t = 0; t < 256; t++)
                    for (unsigned u = 0; u < U; u++) {
                        const size_t i = c * 256 * U + t + (size_t)u * 256;
                        if (i >= A.nv) continue;
                        for (size_t k = 0; k < EPV; k++)
                            if (!hit(cnt, A.head + i * EPV + k)) return fail("tree: vector past the end", n, mo, mx);
                    }
            continue;
        }
        const size_t tail0 = A.head + A.nv * EPV, nscalar = A.head + (A.n - tail0);
        const size_t stride = (size_t)(nblocks - A.nvb) * 256;
        for (unsigned t = 0; t < 256; t++)
            for (size_t k = (size_t)(b - A.nvb) * 256 + t; k < nscalar; k += stride)
                if (!hit(cnt, k < A.head ? k : tail0 + (k - A.head))) return fail("tree: element past the end", n, mo, mx);
    }
    for (size_t e = 0; e < n; e++)
        if (cnt[e] != 1) return fail(cnt[e] ? "tree: element written twice" : "tree: element never written", n, mo, mx);
    if (mo == mx && mo % ES == 0 && n >= 2 * EPV && !A.nv) return fail("tree: co-aligned sources without a vector body", n, mo, mx);
    if ((mo != mx || mo % ES) && A.nv) return fail("tree: a vector body on sources that are not co-aligned", n, mo, mx);
    return 0;
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

// the one-shot form: p trees over consecutive windows of one vector (Raben's blocks, which
// fall on odd element offsets), then the same batch capped to few workgroups
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

int main()
{
    long cases = 0;
    for (size_t es : {(size_t)8, (size_t)16}) {
        ES = es;
        EPV = 16 / es;
        const unsigned step = es == 8 ? 4 : 8; // the alignment of the type's C layout
        for (size_t n : kSizes)
            for (unsigned mo = 0; mo < 16; mo += step)
                for (unsigned mx = 0; mx < 16; mx += step) {
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
    }
    printf("OK %ld cases\n", cases);
    return 0;
}
