// planmixed_check.cpp -- TEST: host-side check of the mixed gather / scatter kernel's tile -> entry
// -> piece walk (ftar::gather_first, and per entry ftar::cvt_piece for a 2-byte type or
// ftar::gather_piece with es = 4 for float32, as gather_mix_kernel chooses in ftar_kernels.hip).
//
// The grid is laid out in packed (float32) space, one workgroup per 16 KiB tile = 4096 elements of
// any type.  This program replays the walk on the host over tables of mixed types -- neighbours of
// different types at every user offset of 0 .. 7 elements, the sizes 1, 3, 5, 255, 256, 257, 4093,
// 4099 and 8193, 1024 tiny entries, capped grids -- and turns every piece into the accesses the
// kernel makes for it.  It asserts that every packed byte and every user byte is touched exactly
// once, that packed and user positions correspond element for element, and that no access is
// misaligned to its width on either side.  No GPU needed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../fault-tolerant_amd/csrc/ftar_kernels.h"

using namespace ftar;

static long g_pieces = 0, g_f32_vec = 0, g_cvt_wide = 0;
static const uintptr_t kPacked = (uintptr_t)1 << 40; // 256-byte aligned, as the staging allocation

struct Table {
    std::vector<GEntry> e;
    std::vector<unsigned> ty;
};

static unsigned ues(unsigned dt) { return dt == (unsigned)kFloat32 ? 4 : 2; }

static int fail(const char *what, int n, int e, unsigned grid)
{
    fprintf(stderr, "%d entries, entry %d, grid %u: %s\n", n, e, grid, what);
    return 1;
}

// one access of `w` elements starting at element j of the piece (first element at ua / poff)
static int touch(const Table &T, int e, uintptr_t ua0, size_t poff0, size_t j, unsigned w, unsigned pw, std::vector<uint8_t> &pc,
                 std::vector<std::vector<uint8_t>> &uc, unsigned grid)
{
    const unsigned us = ues(T.ty[e]);
    const uintptr_t ua = ua0 + us * j, pa = kPacked + poff0 + 4 * j;
    const int n = (int)T.e.size();
    if (ua % (us * w)) return fail("user access not aligned to its width", n, e, grid);
    if (pa % pw) return fail("packed access not aligned to its width", n, e, grid); // (k = 8: two 16-byte accesses)
    for (unsigned i = 0; i < w; i++) {
        const size_t pel = (poff0 + 4 * (j + i)) / 4;
        const size_t uel = (ua + us * i - (uintptr_t)T.e[e].ptr) / us;
        if (pel - T.e[e].off / 4 != uel) return fail("packed element from the wrong user element", n, e, grid);
        for (unsigned b = 0; b < 4; b++) pc[4 * pel + b]++;
        for (unsigned b = 0; b < us; b++) uc[e][us * uel + b]++;
    }
    return 0;
}

static int walk(const Table &T, unsigned grid)
{
    const int n = (int)T.e.size();
    const size_t total = T.e[n - 1].off + T.e[n - 1].bytes;
    const unsigned ntiles = (unsigned)((total + kTileBytes - 1) / kTileBytes);
    if (grid > ntiles) grid = ntiles;
    std::vector<uint8_t> pc(total, 0);
    std::vector<std::vector<uint8_t>> uc(n);
    for (int i = 0; i < n; i++) uc[i].assign(T.e[i].bytes / 4 * ues(T.ty[i]), 0);
    for (unsigned b = 0; b < grid; b++)
        for (unsigned t = b; t < ntiles; t += grid) {
            const size_t lo = (size_t)t * kTileBytes, hi = lo + kTileBytes < total ? lo + kTileBytes : total;
            int e = gather_first(T.e.data(), n, lo);
            if (e < 0 || e >= n || T.e[e].off > lo || T.e[e].off + T.e[e].bytes <= lo)
                return fail("the search did not find the entry holding the tile's first byte", n, e, grid);
            for (; e < n; e++) {
                const GEntry &E = T.e[e];
                const size_t pb = E.off > lo ? E.off : lo, pe = E.off + E.bytes < hi ? E.off + E.bytes : hi;
                if (pb >= pe) break;
                g_pieces++;
                if (T.ty[e] == (unsigned)kFloat32) {
                    GPiece P;
                    if (!gather_piece(E, lo, hi, (const char *)kPacked, 4, &P)) return fail("no piece where the kernel expects one", n, e, grid);
                    if (P.poff != pb || P.bytes != pe - pb || P.unit != 4 || P.head % 4 || P.bytes % 4)
                        return fail("float32 piece: bounds or unit", n, e, grid);
                    const uintptr_t ua = (uintptr_t)P.user;
                    size_t j = 0;
                    for (; j < P.head / 4; j++)
                        if (touch(T, e, ua, P.poff, j, 1, 4, pc, uc, grid)) return 1;
                    if (P.vec) {
                        g_f32_vec += (long)P.nvec;
                        for (size_t v = 0; v < P.nvec; v++, j += 4)
                            if (touch(T, e, ua, P.poff, j, 4, 16, pc, uc, grid)) return 1;
                    } else if (P.nvec || P.head != P.bytes) {
                        return fail("unaligned float32 piece not all word by word", n, e, grid);
                    }
                    for (; j < P.bytes / 4; j++)
                        if (touch(T, e, ua, P.poff, j, 1, 4, pc, uc, grid)) return 1;
                } else {
                    CPiece P;
                    if (!cvt_piece(E, lo, hi, (const char *)kPacked, &P)) return fail("no piece where the kernel expects one", n, e, grid);
                    if (P.poff != pb || 4 * P.n != pe - pb) return fail("2-byte piece: bounds", n, e, grid);
                    const uintptr_t ua = (uintptr_t)P.user;
                    if (P.k == 8) g_cvt_wide++;
                    size_t j = 0;
                    for (; j < P.head; j++)
                        if (touch(T, e, ua, P.poff, j, 1, 4, pc, uc, grid)) return 1;
                    for (size_t g = 0; g < P.nvec; g++, j += P.k)
                        if (touch(T, e, ua, P.poff, j, P.k, P.k == 8 ? 16 : 4 * P.k, pc, uc, grid)) return 1;
                    for (; j < P.n; j++)
                        if (touch(T, e, ua, P.poff, j, 1, 4, pc, uc, grid)) return 1;
                }
                if (E.off + E.bytes >= hi) { // the kernel's early exit: the tile ends inside this entry
                    e++;
                    break;
                }
            }
            if (e < n && T.e[e].off < hi) return fail("walk stopped inside the tile", n, e, grid);
        }
    for (size_t k = 0; k < pc.size(); k++)
        if (pc[k] != 1) return fail("a packed byte not touched exactly once", n, -1, grid);
    for (int i = 0; i < n; i++)
        for (size_t k = 0; k < uc[i].size(); k++)
            if (uc[i][k] != 1) return fail("a user byte not touched exactly once", n, i, grid);
    return 0;
}

static const unsigned kCycle[3] = {(unsigned)kBFloat16, (unsigned)kFloat32, (unsigned)kFloat16};

// entries of the given element counts, types cycling from `first`, entry i's user pointer
// `mis(i)` ELEMENTS past a 16-byte boundary
template <typename F> static Table table(const std::vector<size_t> &counts, unsigned first, F mis)
{
    Table T;
    size_t off = 0;
    for (size_t i = 0; i < counts.size(); i++) {
        if (!counts[i]) continue;
        const unsigned dt = kCycle[(i + first) % 3];
        const uintptr_t user = ((uintptr_t)2 << 40) + ((uintptr_t)i << 28) + (uintptr_t)mis((int)i) * ues(dt);
        T.e.push_back(GEntry{(void *)user, off, counts[i] * 4});
        T.ty.push_back(dt);
        off += counts[i] * 4;
    }
    return T;
}

int main()
{
    const unsigned grids[] = {1, 2, 3, 7, 1u << 20};
    const size_t tile = kTileBytes / 4;
    std::vector<std::vector<size_t>> lists = {
        {1},
        {1, 3, 0, 5, 255, 256, 257, 4093, 4099, 8193},
        {8193, 4099, 4093, 257, 256, 255, 5, 3, 1},
        {tile, tile, 2 * tile},
        {tile - 1, 1, tile + 1, tile - 1},
        {5, 3 * tile, 1, 1, tile - 7, 7 * tile + 3, 2},
        {8, 16, 24, tile - 48, 8},
    };
    std::vector<size_t> tiny, many(1024);
    for (int i = 0; i < 40; i++) tiny.push_back(1 + (size_t)(i * 5 % 7));
    lists.push_back(tiny);
    for (int i = 0; i < 1024; i++) many[(size_t)i] = 1 + (size_t)(i * 11 % 7); // the largest table, tiny entries
    lists.push_back(many);
    for (const auto &counts : lists)
        for (unsigned grid : grids)
            for (unsigned first = 0; first < 3; first++) {
                for (unsigned m = 0; m < 8; m++) // every entry at the same user offset, 0 .. 7 elements
                    if (walk(table(counts, first, [&](int) { return m; }), grid)) return 1;
                for (int o = 0; o < 8; o++)      // every entry at its own, as the GPU tests' buffers
                    if (walk(table(counts, first, [&](int i) { return (unsigned)((i + o) % 8); }), grid)) return 1;
                {                               // user element congruent to the packed element mod 8: the wide paths
                    Table T = table(counts, first, [&](int) { return 0u; });
                    for (size_t i = 0; i < T.e.size(); i++) T.e[i].ptr = (char *)T.e[i].ptr + (T.e[i].off / 4 % 8) * ues(T.ty[i]);
                    if (walk(T, grid)) return 1;
                }
            }
    if (g_f32_vec == 0 || g_cvt_wide == 0) {
        fprintf(stderr, "a wide path was never taken\n");
        return 1;
    }
    printf("OK %ld pieces, %ld float32 vectors, %ld 2-byte pieces on the widest path\n", g_pieces, g_f32_vec, g_cvt_wide);
    return 0;
}
