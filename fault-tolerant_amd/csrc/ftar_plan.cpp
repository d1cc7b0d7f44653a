// ftar_plan.cpp -- the launch planners of ftar_kernels.hip: heads, bodies, tails, grids and caps.
//
// Host arithmetic only (no HIP call, no device code): what the kernels of ftar_kernels.hip are
// launched over.  A translation unit of its own so that the host checkers (tests/kernel_plan)
// compile it themselves, plain and under ASan + UBSan, without the kernel object.  kBlock,
// kUnroll and the tile constants are ftar_kernels.h's: one definition for kernels and planners.

#include <stdint.h>
#include <string.h>

#include "ftar_kernels.h"

namespace ftar {

unsigned plan_tree(TreeArgs *A, int p, size_t esize, unsigned max_blocks)
{
    uintptr_t mis = (uintptr_t)A->out & 15;
    bool co = (16 % esize == 0) && (mis % esize == 0);
    for (int j = 0; j < p; j++) co = co && (((uintptr_t)A->src[j] & 15) == mis);
    for (int o = 0; o < A->nmore; o++) co = co && (((uintptr_t)A->more[o] & 15) == mis);
    A->head = A->nv = 0;
    if (co) {
        size_t head = mis ? (16 - mis) / esize : 0;
        if (head > A->n) head = A->n;
        A->head = head;
        A->nv = (A->n - head) * esize / 16;
    }
    size_t nscalar = A->n - A->nv * (16 / esize);
    const unsigned u = (A->unroll == 2 || A->unroll == 4) && (p == 4 || p == 8) ? A->unroll : 1;
    A->unroll = u;
    size_t vb = (A->nv + (size_t)kBlock * u - 1) / ((size_t)kBlock * u);
    if (vb > max_blocks) return 0; // the caller splits larger blocks
    size_t sb = (nscalar + kBlock - 1) / kBlock;
    if (sb > 256) sb = 256;
    A->nvb = (unsigned)vb;
    return (unsigned)(vb + sb);
}

unsigned plan_tree_batch(TreeBatch *B, int p, size_t esize, unsigned max_blocks)
{
    unsigned total = 0;
    for (int k = 0; k < B->nt; k++) {
        B->first[k] = total;
        B->t[k].unroll = 1; // tree_batch_kernel is instantiated for one vector per lane and source
        unsigned g = plan_tree(&B->t[k], p, esize, max_blocks);
        if (g == 0) return 0;
        total += g;
    }
    B->first[B->nt] = total;
    return total;
}

unsigned cap_tree_batch(TreeBatch *B, unsigned max_total)
{
    unsigned sb = 0, vb = 0, trees_v = 0;
    for (int k = 0; k < B->nt; k++) {
        vb += B->t[k].nvb;
        sb += B->first[k + 1] - B->first[k] - B->t[k].nvb;
        trees_v += B->t[k].nvb > 0;
    }
    if (vb + sb <= max_total) return vb + sb;
    if (sb + trees_v > max_total) return 0;
    const unsigned avail = max_total - sb;
    unsigned nvb[kMaxBatch], total = 0;
    for (int k = 0; k < B->nt; k++) {
        nvb[k] = B->t[k].nvb ? (unsigned)((unsigned long long)B->t[k].nvb * avail / vb) : 0;
        if (B->t[k].nvb && nvb[k] < 1) nvb[k] = 1;
        total += nvb[k] + (B->first[k + 1] - B->first[k] - B->t[k].nvb);
    }
    if (total > max_total) return 0; // unchanged
    total = 0;
    for (int k = 0; k < B->nt; k++) {
        const unsigned s = B->first[k + 1] - B->first[k] - B->t[k].nvb;
        B->first[k] = total;
        B->t[k].nvb = nvb[k];
        total += nvb[k] + s;
    }
    B->first[B->nt] = total;
    return total;
}

// Split user segments into co-aligned vector bodies + scalar heads/tails and assign
// blocks.  Returns the grid size (0 if there is nothing to do).
unsigned plan_segments(const SegIn *in, int nin, size_t esize, unsigned max_blocks, KSegList *L)
{
    L->nseg = 0;
    L->nt_store = 0;
    L->sig = KSignal{nullptr, nullptr, 0, 0};
    size_t vec_bytes_total = 0;
    struct Piece { KSeg k; size_t bytes; } pieces[kMaxKSegs];
    int np = 0;
    for (int s = 0; s < nin; s++) {
        const SegIn &g = in[s];
        if (g.n == 0) continue;
        uintptr_t ao = (uintptr_t)g.out, ax = (uintptr_t)g.x, ay = (uintptr_t)(g.kind == kCopy ? g.x : g.y);
        uintptr_t ao2 = g.out2 ? (uintptr_t)g.out2 : ao;
        bool co = ((ao & 15) == (ax & 15)) && ((ao & 15) == (ay & 15)) && ((ao & 15) == (ao2 & 15)) &&
                  (16 % esize == 0) && ((ao & 15) % esize == 0);
        size_t head = 0, body = 0;
        if (co) {
            size_t mis = ao & 15;
            head = mis ? (16 - mis) / esize : 0;
            if (head > g.n) head = g.n;
            size_t rest = g.n - head;
            size_t epv = 16 / esize;
            body = (rest / epv) * epv;
        }
        size_t tail_off = head + body;
        auto add = [&](size_t off, size_t n, unsigned vec) {
            if (n == 0) return;
            KSeg k;
            k.out = (char *)g.out + off * esize;
            k.out2 = g.out2 ? (void *)((char *)g.out2 + off * esize) : nullptr;
            k.x = (const char *)g.x + off * esize;
            k.y = g.kind == kCopy ? k.x : (const void *)((const char *)g.y + off * esize);
            k.n = n;
            k.kind = (unsigned)g.kind;
            k.vec = vec;
            k.blk_begin = k.blk_end = 0;
            pieces[np].k = k;
            pieces[np].bytes = n * esize;
            if (vec) vec_bytes_total += n * esize;
            np++;
        };
        add(0, head, 0);
        add(head, body, 1);
        add(tail_off, g.n - tail_off, 0);
    }
    if (np == 0) return 0;
    const size_t tile_bytes = (size_t)kBlock * 16 * kUnroll;
    size_t total_tiles = 0;
    for (int i = 0; i < np; i++)
        if (pieces[i].k.vec) total_tiles += (pieces[i].bytes + tile_bytes - 1) / tile_bytes;
    L->nil = 0;
    L->il_blocks = 0;
    if (total_tiles + 64 * (size_t)np <= max_blocks) {
        // uncapped grid: one block per tile.  Vector pieces of at least one chunk share
        // an interleaved prefix of `rounds` chunks each (the shortest one's length).
        size_t rounds = SIZE_MAX;
        unsigned char il[kMaxIleave];
        int nil = 0;
        for (int i = 0; i < np && nil < kMaxIleave; i++) {
            if (!pieces[i].k.vec) continue;
            size_t t = (pieces[i].bytes + tile_bytes - 1) / tile_bytes;
            if (t < (size_t)kChunkTiles) continue;
            il[nil++] = (unsigned char)i;
            if (t / kChunkTiles < rounds) rounds = t / kChunkTiles;
        }
        if (nil >= 2) {
            L->nil = nil;
            L->il_blocks = (unsigned)(rounds * kChunkTiles * nil);
            memcpy(L->il, il, sizeof(il));
        } else {
            rounds = 0;
        }
        unsigned next = L->il_blocks;
        for (int i = 0; i < np; i++) {
            KSeg &k = pieces[i].k;
            bool in_il = false;
            for (int t = 0; t < L->nil; t++) in_il |= (L->il[t] == i);
            size_t tiles = k.vec ? (pieces[i].bytes + tile_bytes - 1) / tile_bytes : 0;
            size_t base = in_il ? rounds * kChunkTiles : 0;
            size_t want = k.vec ? tiles - base : (k.n + kBlock - 1) / kBlock;
            if (!k.vec && want > 64) want = 64;
            k.ntiles = (unsigned)tiles;
            k.tile_base = (unsigned)base;
            k.blk_begin = next;
            k.blk_end = next + (unsigned)want;
            next = k.blk_end;
            L->s[L->nseg++] = k;
        }
        return next;
    }
    // capped grid (more than max_blocks tiles): blocks split between the pieces in
    // proportion to their bytes, pieces loop with a block stride; scalar pieces (heads/
    // tails < 16 B, or non-co-aligned slow paths) get up to 64 blocks.
    unsigned next = 0;
    for (int i = 0; i < np; i++) {
        KSeg &k = pieces[i].k;
        size_t want;
        if (k.vec) {
            size_t need = (pieces[i].bytes + tile_bytes - 1) / tile_bytes;
            size_t share = vec_bytes_total ? (size_t)((double)max_blocks * (double)pieces[i].bytes /
                                                     (double)vec_bytes_total) + 1
                                           : 1;
            want = need < share ? need : share;
            k.ntiles = (unsigned)need;
        } else {
            size_t need = (k.n + kBlock - 1) / kBlock;
            want = need < 64 ? need : 64;
            k.ntiles = 0;
        }
        if (want < 1) want = 1;
        k.tile_base = 0;
        k.blk_begin = next;
        k.blk_end = next + (unsigned)want;
        next = k.blk_end;
        L->s[L->nseg++] = k;
    }
    return next;
}

} // namespace ftar
