// planacc32_check.cpp -- TEST: host-side check of the converting gather / scatter kernel's tile ->
// entry -> piece walk (ftar::gather_first, ftar::cvt_piece in ftar_kernels.h).
//
// The kernel lays its grid out in packed (float32) space, one workgroup per 16 KiB tile = 4096
// elements = 8 KiB of user memory, with a stride loop when the grid is capped; a workgroup finds
// the first entry overlapping its tile by binary search and walks the entries that follow.  This
// program replays exactly that walk on the host for crafted tables -- a one-element entry, one
// spanning three and more tiles, 300 one-element entries inside one tile, entries ending exactly
// on a tile edge, every user misalignment 0, 2, .., 14 bytes against every packed offset residue
// mod 32, capped grids -- and turns every piece into the accesses the kernel makes for it (head
// elements, groups of k, tail elements).  It asserts that every packed element is produced exactly
// once from the right user element, that every access is aligned to its width on its own side
// (2 k bytes of user memory, 4 k of packed memory; k = 8: two 16-byte packed accesses), that the
// widest path is taken exactly where the element at which the user address reaches a 16-byte
// boundary has its packed address on a 32-byte boundary (and below it the widest class that
// fits), and that no element straddles a piece.  No GPU needed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../fault-tolerant_amd/csrc/ftar_kernels.h"

using namespace ftar;

static long g_checked = 0, g_wide = 0;
static const uintptr_t kPacked = (uintptr_t)1 << 40; // 256-byte aligned, as the staging allocation

static int fail(const char *what, int n, int e, unsigned grid)
{
    fprintf(stderr, "%d entries, entry %d, grid %u: %s\n", n, e, grid, what);
    return 1;
}

// does class k (elements per access) fit a piece whose first element is at ua / pa?
static bool fits(uintptr_t ua, uintptr_t pa, unsigned k)
{
    const size_t h = ((0 - ua) & (2 * k - 1)) / 2; // elements up to the user boundary of 2 k bytes
    return ((pa + 4 * h) & (4 * k - 1)) == 0;
}

// one access of `w` elements at element j of piece P (entry e): alignment on both sides, and every
// element counted against the packed element it produces
static int touch(const std::vector<GEntry> &tab, int e, const CPiece &P, size_t j, unsigned w, std::vector<uint8_t> &cnt,
                 unsigned grid)
{
    const uintptr_t ua = (uintptr_t)P.user + 2 * j, pa = kPacked + P.poff + 4 * j;
    if (ua % (2 * w)) return fail("user access not aligned to its width", (int)tab.size(), e, grid);
    if (pa % (4 * w)) return fail("packed access not aligned to its width", (int)tab.size(), e, grid);
    for (unsigned i = 0; i < w; i++) {
        const size_t pel = (P.poff + 4 * (j + i)) / 4;                 // packed element
        const size_t uel = (ua + 2 * i - (uintptr_t)tab[e].ptr) / 2;   // element of entry e it comes from
        if (pel - tab[e].off / 4 != uel) return fail("packed element from the wrong user element", (int)tab.size(), e, grid);
        cnt[pel]++;
    }
    return 0;
}

static int walk(const std::vector<GEntry> &tab, unsigned grid)
{
    const int n = (int)tab.size();
    const size_t total = tab[n - 1].off + tab[n - 1].bytes; // packed bytes
    const unsigned ntiles = (unsigned)((total + kTileBytes - 1) / kTileBytes);
    if (grid > ntiles) grid = ntiles;
    std::vector<uint8_t> cnt(total / 4, 0);
    for (unsigned b = 0; b < grid; b++) {
        for (unsigned t = b; t < ntiles; t += grid) {
            const size_t lo = (size_t)t * kTileBytes, hi = lo + kTileBytes < total ? lo + kTileBytes : total;
            int e = gather_first(tab.data(), n, lo);
            if (e < 0 || e >= n || tab[e].off > lo || tab[e].off + tab[e].bytes <= lo)
                return fail("the search did not find the entry holding the tile's first byte", n, e, grid);
            for (; e < n; e++) {
                CPiece P;
                if (!cvt_piece(tab[e], lo, hi, (const char *)kPacked, &P)) break;
                g_checked++;
                const uintptr_t ua = (uintptr_t)P.user, pa = kPacked + P.poff;
                if (P.poff < lo || P.poff + 4 * P.n > hi || P.n == 0) return fail("piece outside its tile", n, e, grid);
                if (P.poff < tab[e].off || P.poff + 4 * P.n > tab[e].off + tab[e].bytes) return fail("piece outside its entry", n, e, grid);
                if ((P.poff - tab[e].off) % 4 || (ua - (uintptr_t)tab[e].ptr) % 2 ||
                    (ua - (uintptr_t)tab[e].ptr) / 2 != (P.poff - tab[e].off) / 4)
                    return fail("an element straddles a piece", n, e, grid);
                // the rule, recomputed: the widest class that fits; 8 exactly where the element at the
                // user's 16-byte boundary has its packed address on a 32-byte boundary
                const size_t h16 = ((0 - ua) & 15) / 2;
                const bool widest = ((pa + 4 * h16) & 31) == 0;
                if ((P.k == 8) != widest) return fail("widest path taken where the rule does not hold (or not taken where it does)", n, e, grid);
                const unsigned want = fits(ua, pa, 8) ? 8 : fits(ua, pa, 4) ? 4 : fits(ua, pa, 2) ? 2 : 1;
                if (P.k != want) return fail("not the widest class that fits", n, e, grid);
                if (P.k == 8) g_wide++;
                if (P.k == 1) {
                    if (P.head != P.n || P.nvec != 0) return fail("unaligned piece not all element by element", n, e, grid);
                } else {
                    if (P.head > P.n || P.head >= P.k || P.head + P.nvec * P.k > P.n || P.n - P.head - P.nvec * P.k >= P.k)
                        return fail("head / groups / tail do not add up", n, e, grid);
                }
                size_t j = 0;
                for (; j < P.head; j++)
                    if (touch(tab, e, P, j, 1, cnt, grid)) return 1;
                for (size_t g = 0; g < P.nvec; g++, j += P.k)
                    if (touch(tab, e, P, j, P.k, cnt, grid)) return 1;
                for (; j < P.n; j++)
                    if (touch(tab, e, P, j, 1, cnt, grid)) return 1;
                if (tab[e].off + tab[e].bytes >= hi) { // the kernel's early exit: the tile ends inside this entry
                    e++;
                    break;
                }
            }
            if (e < n && tab[e].off < hi) return fail("walk stopped inside the tile", n, e, grid);
        }
    }
    for (size_t k = 0; k < cnt.size(); k++)
        if (cnt[k] != 1) {
            fprintf(stderr, "packed element %zu produced %u times\n", k, cnt[k]);
            return fail("coverage", n, -1, grid);
        }
    return 0;
}

// entries of the given element counts, entry i's user pointer `mis(i)` bytes past a 16-byte boundary
template <typename F> static std::vector<GEntry> table(const std::vector<size_t> &counts, F mis)
{
    std::vector<GEntry> t;
    size_t off = 0;
    for (size_t i = 0; i < counts.size(); i++) {
        if (!counts[i]) continue;
        const uintptr_t user = ((uintptr_t)2 << 40) + ((uintptr_t)i << 28) + mis((int)i);
        t.push_back(GEntry{(void *)user, off, counts[i] * 4});
        off += counts[i] * 4;
    }
    return t;
}

int main()
{
    const unsigned grids[] = {1, 2, 3, 7, 1u << 20};
    const size_t tile = kTileBytes / 4; // elements per tile
    std::vector<std::vector<size_t>> lists = {
        {1},                                            // a one-element entry
        {3 * tile + 5},                                 // spans four tiles
        {1, 3, 0, 5, 4093, 4099, 8193, 2, 2},           // the GPU test's list
        {tile, tile, 2 * tile},                         // entries ending exactly on tile edges
        {tile - 1, 1, tile + 1, tile - 1},              // ... and one element before / after them
        {5, 3 * tile, 1, 1, tile - 7, 7 * tile + 3, 2}, // long entries between short ones
        {8, 16, 24, tile - 48, 8},                      // multiples of 8 elements: the widest class throughout
    };
    std::vector<size_t> ones(300, 1), tiny;             // 300 one-element entries inside one tile
    lists.push_back(ones);
    for (int i = 0; i < 40; i++) tiny.push_back(1 + (size_t)(i * 5 % 7));
    lists.push_back(tiny);
    std::vector<size_t> many(1024);                     // the largest table
    for (int i = 0; i < 1024; i++) many[(size_t)i] = 1 + (size_t)(i * 11 % 7);
    lists.push_back(many);
    for (const auto &counts : lists)
        for (unsigned grid : grids) {
            for (unsigned m = 0; m < 16; m += 2) // every entry at the same misalignment
                if (walk(table(counts, [&](int) { return m; }), grid)) return 1;
            // every entry at its own, (i + offset) % 8 elements past a boundary as the GPU tests' buffers
            for (int o = 0; o < 2; o++)
                if (walk(table(counts, [&](int i) { return 2u * (unsigned)((i + o) % 8); }), grid)) return 1;
            // user element congruent to the packed element mod 8 (the widest path wherever it can be)
            {
                std::vector<GEntry> t = table(counts, [&](int) { return 0u; });
                for (GEntry &g : t) g.ptr = (char *)g.ptr + (g.off / 4 % 8) * 2;
                if (walk(t, grid)) return 1;
            }
        }
    // every user misalignment 0, 2, .., 14 against every packed offset residue mod 32 (4 * first)
    for (unsigned m = 0; m < 16; m += 2)
        for (size_t first = 1; first <= 8; first++) {
            std::vector<size_t> counts = {first, 8192 + 3, 7};
            if (walk(table(counts, [&](int) { return m; }), 2)) return 1;
        }
    if (g_wide == 0) {
        fprintf(stderr, "no piece took the widest path\n");
        return 1;
    }
    printf("OK %ld pieces, %ld on the widest path\n", g_checked, g_wide);
    return 0;
}
