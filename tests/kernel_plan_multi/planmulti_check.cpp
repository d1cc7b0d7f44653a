// planmulti_check.cpp -- TEST: host-side coverage check of the gather / scatter kernel's tile ->
// entry mapping (ftar::gather_first, ftar::gather_piece in ftar_kernels.h).
//
// The kernel lays its grid out in packed space, one workgroup per 16 KiB tile with a stride loop
// when the grid is capped; a workgroup finds the first entry overlapping its tile by binary
// search and walks the entries that follow.  This program replays exactly that walk on the host
// for crafted tables -- an entry smaller than one vector, one spanning three and more tiles, 300
// one-element entries inside one tile, entries ending exactly on a tile edge, every misalignment
// 0..15 bytes of the user pointer against the packed offset, element sizes 2, 4, 8, 16, capped
// grids -- and asserts that every packed byte is covered exactly once by the right user byte,
// that the 16-byte path is taken exactly where user and packed address are congruent mod 16
// (with aligned vector accesses inside the piece), and that heads, tails and unaligned pieces
// move in units both addresses are aligned to.  No GPU needed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../fault-tolerant_amd/csrc/ftar_kernels.h"

using namespace ftar;

static long g_checked = 0;
static const uintptr_t kPacked = (uintptr_t)1 << 40; // 256-byte aligned, as the staging allocation

static int fail(const char *what, unsigned es, int n, int e, unsigned grid)
{
    fprintf(stderr, "esize %u, %d entries, entry %d, grid %u: %s\n", es, n, e, grid, what);
    return 1;
}

// tab[i].ptr = user base of entry i; user memory of entry i is modelled as the id (i, byte)
static int walk(const std::vector<GEntry> &tab, unsigned es, unsigned grid)
{
    const int n = (int)tab.size();
    const size_t total = tab[n - 1].off + tab[n - 1].bytes;
    const unsigned ntiles = (unsigned)((total + kTileBytes - 1) / kTileBytes);
    if (grid > ntiles) grid = ntiles;
    std::vector<uint8_t> cnt(total, 0);
    for (unsigned b = 0; b < grid; b++) {
        for (unsigned t = b; t < ntiles; t += grid) {
            const size_t lo = (size_t)t * kTileBytes, hi = lo + kTileBytes < total ? lo + kTileBytes : total;
            int e = gather_first(tab.data(), n, lo);
            if (e < 0 || e >= n || tab[e].off > lo || tab[e].off + tab[e].bytes <= lo)
                return fail("the search did not find the entry holding the tile's first byte", es, n, e, grid);
            for (; e < n; e++) {
                GPiece P;
                if (!gather_piece(tab[e], lo, hi, (const char *)kPacked, es, &P)) break;
                g_checked++;
                const uintptr_t ua = (uintptr_t)P.user, pa = kPacked + P.poff;
                if (P.poff < lo || P.poff + P.bytes > hi || P.bytes == 0) return fail("piece outside its tile", es, n, e, grid);
                if (ua - (uintptr_t)tab[e].ptr != P.poff - tab[e].off || P.poff + P.bytes > tab[e].off + tab[e].bytes)
                    return fail("piece outside its entry", es, n, e, grid);
                if (P.bytes % es || (P.poff - tab[e].off) % es) return fail("an element straddles a piece", es, n, e, grid);
                const bool co = ((ua ^ pa) & 15) == 0;
                if ((P.vec != 0) != co) return fail("vector path taken where not co-aligned (or not taken where it is)", es, n, e, grid);
                if (P.unit == 0 || (P.unit & (P.unit - 1)) || P.unit > 8 || P.unit > es || (ua | pa) % P.unit)
                    return fail("scalar unit not aligned on both sides", es, n, e, grid);
                if (es <= 8 && (ua % es == 0) && P.unit != es) return fail("aligned elements not moved whole", es, n, e, grid);
                size_t body = 0;
                if (P.vec) {
                    if (P.head > P.bytes || P.head + P.nvec * 16 > P.bytes || P.bytes - P.head - P.nvec * 16 >= 16)
                        return fail("head / body / tail do not add up", es, n, e, grid);
                    if (P.nvec && (((pa + P.head) & 15) || ((ua + P.head) & 15))) return fail("vector access not 16-byte aligned", es, n, e, grid);
                    if (P.head % P.unit || (P.bytes - P.head - P.nvec * 16) % P.unit) return fail("head or tail not whole units", es, n, e, grid);
                    body = P.nvec * 16;
                } else if (P.head != P.bytes || P.nvec != 0 || P.bytes % P.unit) {
                    return fail("unaligned piece not all scalar", es, n, e, grid);
                }
                (void)body;
                for (size_t k = 0; k < P.bytes; k++) cnt[P.poff + k]++;
                if (tab[e].off + tab[e].bytes >= hi) { // the kernel's early exit: the tile ends inside this entry
                    e++;
                    break;
                }
            }
            // the walk ended: the next entry, if any, starts at or past the tile's end
            if (e < n && tab[e].off < hi) return fail("walk stopped inside the tile", es, n, e, grid);
        }
    }
    for (size_t k = 0; k < total; k++)
        if (cnt[k] != 1) {
            fprintf(stderr, "packed byte %zu covered %u times\n", k, cnt[k]);
            return fail("coverage", es, n, -1, grid);
        }
    return 0;
}

// entries of the given element counts, entry i's user pointer `mis(i)` bytes past a 16-byte boundary
template <typename F> static std::vector<GEntry> table(const std::vector<size_t> &counts, unsigned es, F mis)
{
    std::vector<GEntry> t;
    size_t off = 0;
    for (size_t i = 0; i < counts.size(); i++) {
        if (!counts[i]) continue;
        const uintptr_t user = ((uintptr_t)2 << 40) + ((uintptr_t)i << 28) + mis((int)i);
        t.push_back(GEntry{(void *)user, off, counts[i] * es});
        off += counts[i] * es;
    }
    return t;
}

int main()
{
    const unsigned grids[] = {1, 2, 3, 7, 1u << 20};
    for (unsigned es : {2u, 4u, 8u, 16u}) {
        const size_t tile = kTileBytes / es; // elements per tile
        std::vector<std::vector<size_t>> lists = {
            {1},                                           // smaller than one vector (es < 16)
            {3 * tile + 5},                                // spans four tiles
            {1, 3, 0, 5, 4093, 4099, 8193, 2, 2},          // the GPU test's list
            {tile, tile, 2 * tile},                        // entries ending exactly on tile edges
            {tile - 1, 1, tile + 1, tile - 1},             // ... and one element before / after them
            {5, 3 * tile, 1, 1, tile - 7, 7 * tile + 3, 2}, // long entries between short ones
        };
        std::vector<size_t> ones(300, 1), tiny;            // 300 one-element entries inside one tile
        lists.push_back(ones);
        for (int i = 0; i < 40; i++) tiny.push_back(1 + (size_t)(i * 5 % 7));
        lists.push_back(tiny);
        std::vector<size_t> many(1024);                    // the largest table
        for (int i = 0; i < 1024; i++) many[(size_t)i] = 1 + (size_t)(i * 11 % 7);
        lists.push_back(many);
        const unsigned align = es < 8 ? es : (es == 8 ? 4 : 8); // what the element type's alignment allows
        for (const auto &counts : lists)
            for (unsigned grid : grids) {
                for (unsigned m = 0; m < 16; m += align) // every entry at the same misalignment
                    if (walk(table(counts, es, [&](int) { return m; }), es, grid)) return 1;
                // every entry at its own: packed offset and user pointer then disagree in every way
                if (walk(table(counts, es, [&](int i) { return (unsigned)(i * 7 % 16) / align * align; }), es, grid)) return 1;
                // user pointer congruent to the packed offset (the vector path wherever it can be)
                {
                    std::vector<GEntry> t = table(counts, es, [&](int) { return 0u; });
                    for (GEntry &g : t) g.ptr = (char *)g.ptr + (g.off & 15);
                    if (walk(t, es, grid)) return 1;
                }
            }
    }
    // every misalignment 0..15 of the user pointer against packed offsets 0..15, byte elements' worth
    for (unsigned m = 0; m < 16; m += 2)
        for (size_t first = 1; first <= 9; first++) {
            std::vector<size_t> counts = {first, 8192 + 3, 7};
            if (walk(table(counts, 2, [&](int) { return m; }), 2, 2)) return 1;
        }
    printf("OK %ld pieces\n", g_checked);
    return 0;
}
