// TEST-ONLY, host-only (no HIP call): the reference of ref_types.h as a program, and the
// self-test of the inputs of gen_types.h (tests/test_kernel_ref.py runs both, and once more a
// build of this file with the host sanitizers).
//
//   ref_check apply DTYPE OP IN INOUT OUT   OUT = INOUT op IN, element-wise, over whole files
//   ref_check selftest                      generates the inputs of every case of tree_check's and
//       seg_check's `types` matrices, computes the expectations with the reference and asserts:
//       * every 16-bit SUM / PROD case of n >= 257 expects at least one element that a kernel
//         rounding toward zero, rounding ties away from zero, or flushing subnormal results to
//         zero would get wrong (the same tree with that mutant of the rounding differs);
//       * every 16-bit MAX / MIN, FTAR_FLOAT_INT and FTAR_DOUBLE_INT case of n >= 257 expects at
//         least one byte that changes when the operands of every combination are swapped, and no
//         FTAR_2INT case any (its bytes are value and index: nothing else to tell);
//       * in no SUM / PROD case more than 1/8 of the expected elements are NaN (compared by
//         NaN-ness only), and at least half are finite and non-zero.
//     A case is one tree (tree_kernel case, tree of a batch) or one reduce piece of a list.
//       Then the tables of gather_check and the cases of lds_check (gen_movers.h):
//       * every table is replayed with the product's own host functions (gather_first, gather_piece,
//         cvt_piece of ftar_kernels.h; the arenas modelled as 256-byte aligned constants) at the
//         three grids, and what the matrices are meant to reach is counted -- every unit of the
//         plain mover, vector pieces with head, body and tail, pieces that are not vector pieces,
//         small pieces on each of the four waves, the unrolled loops and their remainders and exact
//         ends, tiles ending inside an entry and exactly at one's end, workgroups with two tiles
//         and more, the converting classes 8, 4, 2 with head and tail and class 1.  Every count
//         that the kernels can reach must be non-zero (the plain mover's one-wave pieces hold at
//         most 63 vectors: its unrolled loop needs the workgroup).  The replay is accounting only:
//         gather_check's expectation is plain concatenation.
//       * every converting scatter case (table x type x scale) of 257 elements and more at a scale
//         other than 0 expects at least one element that rounding toward zero, ties away from zero
//         or flushed subnormals would get wrong, and at the scales whose product is not exact in
//         float32 one that a single rounding of the exact product (a fused multiply-convert) would;
//         over the matrix, a +0 for a zero product and an infinity for a NaN whose upper 16 bits
//         read as one are seen, and -0 is expected both in elements that move one by one and in
//         elements of a packed group, for both types;
//       * in no such case (the block of infinities and NaNs apart) more than 1/8 of the expected
//         elements are NaN, and at least half are finite and non-zero except at scale 0;
//       * every order-sensitive lds_check case expects, in its full tiles and in its ragged rest
//         alike (where they hold 257 elements or more), a byte that swapped operands would change;
//       * the mixed tables (gather_check mix) are replayed the same way with every entry going by
//         its own type, as in gather_mix_kernel, and must reach, for each of the three types, a
//         workgroup's piece, a small piece on each wave, a tile ending inside an entry and at its
//         end with each other type behind it, a piece in a workgroup's second tile or later and
//         pieces of exactly 1020 / 1024 / 1028 packed bytes; every ordered pair of neighbouring
//         types inside one tile; every converting class for both 2-byte types; for float32 a
//         vector piece with body, tail and a head of 1, 2 and 3 words, a piece that is not a vector
//         piece, the unrolled loop at 256 threads and its remainder, nvec = 1023 and 1024, a word
//         loop at 64 and at 256 threads; a pinned table and one of 1024 entries;
//       * every mixed scatter case (table x scale, scale not 0) meets the converting conditions on
//         its 2-byte elements where it has 257 of them, and where it has 257 float32 elements
//         expects one that a subnormal product flushed to zero would change and, unless the scale
//         is 1, one that a missing multiplication would; over the matrix both of these and a -0
//         product that a +0 would miss occur in an element that moves as a word and in one that
//         moves in a 16-byte vector, -0 alone and in a group for both 2-byte types, a NaN whose
//         upper half reads as an infinity, and among the float32 words to gather a signalling NaN
//         in a word and in a vector; the NaN and finite shares hold as above.
//   ref_check narrow DTYPE IN OUT   OUT = the float32 file IN narrowed once (the reference of the
//       converting scatter at scale 1), 2 bytes per element
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "ftar_kernels.h"
#include "gen_movers.h"
#include "gen_types.h"

using namespace kgen;

static Bytes read_file(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        perror(path);
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    Bytes b((size_t)sz);
    if (sz && fread(b.data(), 1, (size_t)sz, f) != (size_t)sz) {
        perror(path);
        exit(2);
    }
    fclose(f);
    return b;
}

static int apply(int dt, int op, const char *fin, const char *finout, const char *fout)
{
    const Bytes in = read_file(fin);
    Bytes inout = read_file(finout);
    const size_t es = esize(dt);
    if (in.size() != inout.size() || in.size() % es) {
        fprintf(stderr, "ref_check: operand files of %zu and %zu bytes, element size %zu\n", in.size(), inout.size(), es);
        return 2;
    }
    const int rc = reduce_local(dt, op, in.data(), inout.data(), in.size() / es);
    if (rc) {
        fprintf(stderr, "ref_check: dtype %d op %d refused (%d)\n", dt, op, rc);
        return 2;
    }
    FILE *f = fopen(fout, "wb");
    if (!f || fwrite(inout.data(), 1, inout.size(), f) != inout.size()) {
        perror(fout);
        return 2;
    }
    fclose(f);
    return 0;
}

struct Stats {
    int cases = 0, judged = 0, failed = 0;
    double max_nan = 0, min_finite = 1;
    size_t min_mut[3] = {SIZE_MAX, SIZE_MAX, SIZE_MAX}, min_swap = SIZE_MAX, max_swap_2int = 0;
};

static void fail(Stats &S, const char *what, const char *why, int dt, int op, int p, size_t n)
{
    S.failed++;
    printf("FAIL %s dtype %d op %d p %d n %zu: %s\n", what, dt, op, p, n, why);
}

// one tree of p sources (a reduce piece: p = 2)
static void judge(Stats &S, const char *what, int dt, int op, int p, size_t n, uint64_t seed)
{
    const Combo c{dt, op};
    const std::vector<Bytes> src = sources(dt, op, n, p, seed);
    const Bytes want = tree_expect(src, p, dt, op, n, false);
    S.cases++;
    if (rounds(c)) {
        size_t nan = 0, fin = 0;
        for (size_t i = 0; i < n; i++) {
            uint16_t w;
            memcpy(&w, &want[2 * i], 2);
            const double v = decode16(w, dt);
            nan += std::isnan(v);
            fin += std::isfinite(v) && v != 0.0;
        }
        const double sn = (double)nan / (double)n, sf = (double)fin / (double)n;
        if (sn > S.max_nan) S.max_nan = sn;
        if (sf < S.min_finite) S.min_finite = sf;
        if (nan * 8 > n) fail(S, what, "more than 1/8 of the expected elements are NaN", dt, op, p, n);
        if (fin * 2 < n) fail(S, what, "fewer than half of the expected elements are finite and non-zero", dt, op, p, n);
        if (n < 257) return;
        S.judged++;
        static const char *names[3] = {"rounding toward zero goes unseen", "ties away from zero go unseen",
                                       "flushed subnormal results go unseen"};
        for (int m = 0; m < 3; m++) {
            const Bytes mut = tree_expect(src, p, dt, op, n, false, (Round)(m + 1));
            const size_t d = count_diff(mut.data(), want.data(), dt, op, n);
            if (d < S.min_mut[m]) S.min_mut[m] = d;
            if (d == 0) fail(S, what, names[m], dt, op, p, n);
        }
        return;
    }
    if (n < 257) return;
    S.judged++;
    const Bytes sw = tree_expect(src, p, dt, op, n, true);
    size_t d = 0;
    for (size_t i = 0; i < want.size(); i++) d += sw[i] != want[i];
    if (order_sensitive(c)) {
        if (d < S.min_swap) S.min_swap = d;
        if (d == 0) fail(S, what, "swapped operands go unseen", dt, op, p, n);
    } else {
        if (d > S.max_swap_2int) S.max_swap_2int = d;
        if (d != 0) fail(S, what, "FTAR_2INT depends on the operand order", dt, op, p, n);
    }
}

// ---------------------------------------------------------------------------------
// the movers' tables (gather_check) and the LDS reduce's cases (lds_check)
// ---------------------------------------------------------------------------------
namespace {
using namespace kmov;

const uintptr_t kDevBase = ((uintptr_t)1 << 40) + (size_t)ftar::kMaxGather * sizeof(ftar::GEntry); // 256-byte aligned
const uintptr_t kHostBase = (uintptr_t)3 << 40;

struct Loops { // one strided loop pair of move_piece / cvt_groups, by thread count (64: index 0, 256: index 1)
    size_t unrolled[2] = {0, 0}, rest[2] = {0, 0}, end_m1[2] = {0, 0}, end_0[2] = {0, 0}, end_p1[2] = {0, 0};
    void add(size_t n, unsigned nth)
    {
        const int w = nth == 256;
        unrolled[w] += n > 3 * (size_t)nth;      // thread 0 enters the loop of kUnroll = 4
        rest[w] += n % (4 * (size_t)nth) != 0;   // some thread has an element left behind it
        end_m1[w] += n == 4 * (size_t)nth - 1;
        end_0[w] += n == 4 * (size_t)nth;
        end_p1[w] += n == 4 * (size_t)nth + 1;
    }
};

struct Cover {
    size_t pieces = 0, unit[4] = {0, 0, 0, 0}, vec_hbt = 0, nonvec = 0, small_wave[4] = {0, 0, 0, 0}, big = 0;
    size_t tile_inside = 0, tile_at_end = 0, wg_two_tiles = 0;
    size_t cls_ht[4] = {0, 0, 0, 0}; // classes 8, 4, 2 with head, body and tail; class 1
    Loops loops;
};

// what only a mixed table can reach; a type is indexed 0: float16, 1: bfloat16, 2: float32
struct MixCover {
    size_t big[3] = {}, small_wave[3][4] = {}, inside[3] = {}, at_end[3][3] = {}, later_tile[3] = {}, next_to[3][3] = {};
    size_t cls_ht[2][4] = {};                                  // per 2-byte type, as Cover's
    size_t f_hbt[4] = {}, f_nonvec = 0, f_words[2] = {0, 0};   // float32: head of 1, 2, 3 words with body and tail; word loops at 64 / 256 threads
    Loops f_loops;                                             // float32: the loops over 16-byte vectors
    size_t threshold[3][3] = {};                               // pieces of exactly 1020, 1024, 1028 packed bytes
};

std::vector<ftar::GEntry> entries(const Table &T, const Layout &L)
{
    std::vector<ftar::GEntry> tab(T.cnt.size());
    for (size_t e = 0; e < tab.size(); e++)
        tab[e] = ftar::GEntry{(void *)((T.pinned ? kHostBase : kDevBase) + L.user_at[e]), L.off[e], T.cnt[e] * T.es};
    return tab;
}

// the kernels' walk; `path` (converting and mixed tables): 1 where an element moves alone (a 2-byte
// element outside a group, a float32 word of a head, a tail or a piece that is not a vector piece),
// 2 in a group or a 16-byte vector.  A mixed table's entry goes by its own type, as in
// gather_mix_kernel: float32 through gather_piece with es = 4, a 2-byte one through cvt_piece, the
// workgroup's piece or a wave's decided from pe - pb.
int replay(const Table &T, unsigned grid, Cover &C, std::vector<unsigned char> *path, MixCover *M = nullptr)
{
    const Layout L = layout(T);
    const std::vector<ftar::GEntry> tab = entries(T, L);
    const char *packed = (const char *)(kDevBase + L.packed_at);
    const int n = (int)tab.size();
    const unsigned ntiles = (unsigned)((L.total + ftar::kTileBytes - 1) / ftar::kTileBytes);
    std::vector<unsigned char> cnt(L.total / T.es, 0);
    for (unsigned b = 0; b < grid; b++) {
        unsigned mine = 0;
        for (unsigned t = b; t < ntiles; t += grid, mine++) {
            const size_t lo = (size_t)t * ftar::kTileBytes, hi = lo + ftar::kTileBytes < L.total ? lo + ftar::kTileBytes : L.total;
            int prev = -1; // the entry in front, where it had a piece in this tile
            for (int e = ftar::gather_first(tab.data(), n, lo); e < n; e++) {
                size_t poff, bytes;
                const int ti = M ? type_index(T.ty[(size_t)e]) : 0;
                if (M) {
                    const size_t pb = tab[e].off > lo ? tab[e].off : lo, pe = tab[e].off + tab[e].bytes < hi ? tab[e].off + tab[e].bytes : hi;
                    if (pb >= pe) break;
                    const bool big = pe - pb >= kWave;
                    if (big) M->big[ti]++;
                    else M->small_wave[ti][e & 3]++;
                    for (int k = 0; k < 3; k++) M->threshold[ti][k] += pe - pb == 1020 + 4 * (size_t)k;
                    M->later_tile[ti] += mine >= 1;
                    if (prev >= 0) M->next_to[type_index(T.ty[(size_t)prev])][ti]++;
                    if (tab[e].off + tab[e].bytes > hi) M->inside[ti]++;
                    else if (tab[e].off + tab[e].bytes == hi && e + 1 < n) M->at_end[ti][type_index(T.ty[(size_t)e + 1])]++;
                }
                prev = e;
                if (T.two_byte((size_t)e)) {
                    ftar::CPiece P;
                    if (!ftar::cvt_piece(tab[e], lo, hi, packed, &P)) break;
                    poff = P.poff;
                    bytes = P.n * 4;
                    const unsigned nth = bytes >= kWave ? 256 : 64;
                    const size_t tail = P.k == 1 ? 0 : P.n - P.head - P.nvec * P.k;
                    C.cls_ht[P.k == 8 ? 0 : P.k == 4 ? 1 : P.k == 2 ? 2 : 3] += P.k == 1 || (P.head && P.nvec && tail);
                    if (M) M->cls_ht[ti][P.k == 8 ? 0 : P.k == 4 ? 1 : P.k == 2 ? 2 : 3] += P.k == 1 || (P.head && P.nvec && tail);
                    C.loops.add(P.head, nth);
                    if (P.k > 1) {
                        C.loops.add(P.nvec, nth);
                        C.loops.add(tail, nth);
                    }
                    if (path)
                        for (size_t i = 0; i < P.n; i++)
                            (*path)[poff / 4 + i] = (P.k == 1 || i < P.head || i >= P.head + P.nvec * P.k) ? 1 : 2;
                } else {
                    ftar::GPiece P;
                    if (!ftar::gather_piece(tab[e], lo, hi, packed, T.es, &P)) break;
                    poff = P.poff;
                    bytes = P.bytes;
                    C.unit[P.unit == 1 ? 0 : P.unit == 2 ? 1 : P.unit == 4 ? 2 : 3]++;
                    C.vec_hbt += P.vec && P.head && P.nvec && P.bytes - P.head - 16 * P.nvec;
                    C.nonvec += !P.vec;
                    const unsigned nth = bytes >= kWave ? 256 : 64;
                    if (M) { // scale_piece / move_piece<false> on words and 16-byte vectors
                        const size_t tail = P.vec ? P.bytes - P.head - 16 * P.nvec : 0;
                        if (P.vec && P.nvec && tail) M->f_hbt[P.head / 4]++;
                        M->f_nonvec += !P.vec;
                        M->f_words[nth == 256] += (P.head != 0) + (tail != 0);
                        if (P.vec) M->f_loops.add(P.nvec, nth);
                        if (path)
                            for (size_t i = 0; i < P.bytes / 4; i++)
                                (*path)[poff / 4 + i] = (!P.vec || 4 * i < P.head || 4 * i >= P.head + 16 * P.nvec) ? 1 : 2;
                    } else if (P.vec) {
                        C.loops.add(P.nvec, nth);
                    }
                }
                C.pieces++;
                if (bytes >= kWave) C.big++;
                else C.small_wave[e & 3]++;
                for (size_t i = 0; i < bytes / T.es; i++) cnt[poff / T.es + i]++;
                if (tab[e].off + tab[e].bytes >= hi) {
                    if (tab[e].off + tab[e].bytes > hi) C.tile_inside++;
                    else if (e + 1 < n) C.tile_at_end++;
                    break;
                }
            }
        }
        C.wg_two_tiles += mine >= 2;
    }
    for (unsigned char c : cnt)
        if (c != 1) {
            printf("FAIL %s grid %u: an element is covered %d times by the replay\n", T.name.c_str(), grid, c);
            return 1;
        }
    return 0;
}

int need(const char *what, size_t v)
{
    if (v) return 0;
    printf("FAIL the movers' tables never reach: %s\n", what);
    return 1;
}

int movers_selftest()
{
    int failed = 0;
    // ---- coverage ----
    Cover P, V;
    size_t nplain = 0, ncvt = 0, pinned[2] = {0, 0};
    for (const Table &T : plain_tables()) {
        nplain++;
        pinned[0] += T.pinned;
        const Layout L = layout(T);
        for (unsigned g : grids((unsigned)((L.total + kTile - 1) / kTile))) failed += replay(T, g, P, nullptr);
    }
    const std::vector<Table> ctab = cvt_tables();
    std::vector<std::vector<unsigned char>> paths;
    for (const Table &T : ctab) {
        ncvt++;
        pinned[1] += T.pinned;
        const Layout L = layout(T);
        paths.emplace_back(T.elems(), 0);
        bool first = true;
        for (unsigned g : grids((unsigned)((L.total + kTile - 1) / kTile))) {
            failed += replay(T, g, V, first ? &paths.back() : nullptr);
            first = false;
        }
    }
    printf("selftest: %zu plain tables (%zu pinned), %zu converting tables (%zu pinned); each runs in both directions\n", nplain,
           pinned[0], ncvt, pinned[1]);
    printf("selftest: plain: %zu pieces; unit 1 / 2 / 4 / 8: %zu / %zu / %zu / %zu; vector pieces with head, body and tail %zu, "
           "not vector %zu\n", P.pieces, P.unit[0], P.unit[1], P.unit[2], P.unit[3], P.vec_hbt, P.nonvec);
    printf("selftest: plain: small pieces on wave 0 / 1 / 2 / 3: %zu / %zu / %zu / %zu, the workgroup's %zu; tiles ending inside an "
           "entry %zu, at an entry's end %zu; workgroups with >= 2 tiles %zu\n", P.small_wave[0], P.small_wave[1], P.small_wave[2],
           P.small_wave[3], P.big, P.tile_inside, P.tile_at_end, P.wg_two_tiles);
    printf("selftest: plain: unrolled loop entered at 64 / 256 threads: %zu / %zu, remainder: %zu / %zu; nvec = 4 * 256 - 1 / + 0: "
           "%zu / %zu\n", P.loops.unrolled[0], P.loops.unrolled[1], P.loops.rest[0], P.loops.rest[1], P.loops.end_m1[1], P.loops.end_0[1]);
    printf("selftest: converting: %zu pieces; class 8 / 4 / 2 with head, groups and tail: %zu / %zu / %zu, class 1: %zu\n", V.pieces,
           V.cls_ht[0], V.cls_ht[1], V.cls_ht[2], V.cls_ht[3]);
    printf("selftest: converting: small pieces on wave 0 / 1 / 2 / 3: %zu / %zu / %zu / %zu, the workgroup's %zu; tiles ending inside "
           "an entry %zu, at an entry's end %zu; workgroups with >= 2 tiles %zu\n", V.small_wave[0], V.small_wave[1], V.small_wave[2],
           V.small_wave[3], V.big, V.tile_inside, V.tile_at_end, V.wg_two_tiles);
    printf("selftest: converting: unrolled loop entered at 64 / 256 threads: %zu / %zu, remainder: %zu / %zu; groups = 4 * 64 - 1: %zu, "
           "4 * 256 - 1 / + 0 / + 1: %zu / %zu / %zu\n", V.loops.unrolled[0], V.loops.unrolled[1], V.loops.rest[0], V.loops.rest[1],
           V.loops.end_m1[0], V.loops.end_m1[1], V.loops.end_0[1], V.loops.end_p1[1]);
    failed += need("a pinned plain table", pinned[0]) + need("a pinned converting table", pinned[1]);
    failed += need("unit 1", P.unit[0]) + need("unit 2", P.unit[1]) + need("unit 4", P.unit[2]) + need("unit 8", P.unit[3]);
    failed += need("a vector piece with head, body and tail", P.vec_hbt) + need("a piece that is not a vector piece", P.nonvec);
    for (const Cover *C : {&P, &V}) {
        for (int w = 0; w < 4; w++) failed += need("a small piece on each wave", C->small_wave[w]);
        failed += need("a piece of the workgroup", C->big) + need("a tile ending inside an entry", C->tile_inside) +
                  need("a tile ending at an entry's end", C->tile_at_end) + need("a workgroup with two tiles", C->wg_two_tiles);
        failed += need("the unrolled loop at 256 threads", C->loops.unrolled[1]) + need("its remainder", C->loops.rest[1]) +
                  need("the remainder loop at 64 threads", C->loops.rest[0]) + need("a count of 4 * 256 - 1", C->loops.end_m1[1]) +
                  need("a count of 4 * 256", C->loops.end_0[1]);
    }
    // (plain one-wave pieces hold at most 63 vectors: the unrolled loop at 64 threads is the converting mover's alone)
    failed += need("the unrolled loop at 64 threads", V.loops.unrolled[0]) + need("4 * 64 - 1 groups", V.loops.end_m1[0]) +
              need("4 * 256 + 1 groups", V.loops.end_p1[1]);
    for (int k = 0; k < 4; k++) failed += need("every converting class with head and tail", V.cls_ht[k]);

    // ---- the scatter inputs against the mutants of the narrowing ----
    static const char *names[4] = {"rounding toward zero goes unseen", "ties away from zero go unseen",
                                   "flushed subnormal results go unseen", "a fused multiply-convert goes unseen"};
    size_t cases = 0, judged = 0, min_mut[4] = {SIZE_MAX, SIZE_MAX, SIZE_MAX, SIZE_MAX}, plus_zero = 0, upper_half = 0;
    size_t neg_zero[2][2] = {{0, 0}, {0, 0}}; // [type][alone, in a group]
    double max_nan = 0, min_finite = 1;
    for (size_t ti = 0; ti < ctab.size(); ti++) {
        const Table &T = ctab[ti];
        const size_t n = T.elems();
        for (int dt : {(int)kFloat16, (int)kBFloat16})
            for (float scale : kScales) {
                cases++;
                size_t nan = 0, fin = 0, mut[4] = {0, 0, 0, 0};
                for (size_t g = 0; g < n; g++) {
                    const float a = cvt_packed(T, dt, scale, g);
                    const uint16_t w = narrow_ref(a, scale, dt);
                    const double v = decode16(w, dt);
                    nan += std::isnan(v);
                    fin += std::isfinite(v) && v != 0.0;
                    if (std::isnan(v)) {
                        upper_half += !is_nan16(narrow_ref(a, scale, dt, kUpperHalf), dt);
                        continue; // compared by NaN-ness: every mutant gives a NaN here as well
                    }
                    for (int m = 0; m < 4; m++) mut[m] += narrow_ref(a, scale, dt, m + 1) != w;
                    if (scale == 0.0f) continue; // (there every negative a gives -0)
                    plus_zero += narrow_ref(a, scale, dt, kPlusZero) != w;
                    if (w == 0x8000) neg_zero[dt == kBFloat16][paths[ti][g] == 2]++;
                }
                const double sn = (double)nan / (double)n, sf = (double)fin / (double)n;
                auto bad = [&](const char *why) {
                    failed++;
                    printf("FAIL %s dtype %d scale %.9g: %s\n", T.name.c_str(), dt, scale, why);
                };
                if (T.block != kNonFinite) {
                    if (sn > max_nan) max_nan = sn;
                    if (nan * 8 > n) bad("more than 1/8 of the expected elements are NaN");
                }
                if (n < 257 || scale == 0.0f) continue;
                if (sf < min_finite) min_finite = sf;
                if (fin * 2 < n) bad("fewer than half of the expected elements are finite and non-zero");
                judged++;
                for (int m = 0; m < 4; m++) {
                    if (m == 3 && exact_scale(scale)) continue;
                    if (mut[m] < min_mut[m]) min_mut[m] = mut[m];
                    if (!mut[m]) bad(names[m]);
                }
            }
    }
    printf("selftest: %zu converting scatter cases, %zu of >= 257 elements at a scale other than 0\n", cases, judged);
    printf("selftest: converting: largest NaN share %.4f, smallest finite non-zero share %.4f\n", max_nan, min_finite);
    printf("selftest: converting: smallest mutant difference (elements): toward zero %zu, ties away %zu, subnormals flushed %zu, "
           "fused %zu\n", min_mut[0], min_mut[1], min_mut[2], min_mut[3]);
    printf("selftest: converting: +0 for a zero product seen in %zu elements, an infinity for a NaN in %zu; -0 expected alone / in a "
           "group: float16 %zu / %zu, bfloat16 %zu / %zu\n", plus_zero, upper_half, neg_zero[0][0], neg_zero[0][1], neg_zero[1][0],
           neg_zero[1][1]);
    failed += need("a -0 that a +0 would miss", plus_zero) + need("a NaN whose upper half reads as an infinity", upper_half);
    for (int t = 0; t < 2; t++)
        failed += need("-0 in an element that moves alone", neg_zero[t][0]) + need("-0 in an element of a group", neg_zero[t][1]);

    // ---- lds_check: the operand roles in the full tiles and in the ragged rest ----
    size_t lds = 0, lds_judged = 0, min_swap = SIZE_MAX;
    for (const LdsCombo &c : lds_combos())
        for (size_t nv : kLdsVecs) {
            lds++;
            if (!lds_order_sensitive(c)) continue;
            const size_t es = esize(c.dt), n = nv * 16 / es, nfull = nv / kLdsTileVecs * kLdsTileVecs * 16 / es;
            Bytes x(n * es), y(n * es);
            lds_fill(x.data(), c.dt, c.op, n, 0, lds_seed(c.dt, c.op, nv));
            lds_fill(y.data(), c.dt, c.op, n, 1, lds_seed(c.dt, c.op, nv));
            Bytes want = x, sw = y;
            if (reduce_local(c.dt, c.op, y.data(), want.data(), n) || reduce_local(c.dt, c.op, x.data(), sw.data(), n)) {
                printf("FAIL lds dtype %d op %d: the reference refused\n", c.dt, c.op);
                failed++;
                continue;
            }
            const size_t part[3] = {0, nfull, n};
            for (int r = 0; r < 2; r++) {
                if (part[r + 1] - part[r] < 257) continue;
                lds_judged++;
                size_t d = 0;
                for (size_t i = part[r] * es; i < part[r + 1] * es; i++) d += want[i] != sw[i];
                if (d < min_swap) min_swap = d;
                if (!d) {
                    printf("FAIL lds dtype %d op %d, %zu vectors: swapped operands go unseen in the %s\n", c.dt, c.op, nv,
                           r ? "ragged rest" : "full tiles");
                    failed++;
                }
            }
        }
    printf("selftest: %zu lds cases; %zu order-sensitive parts of >= 257 elements, smallest swap difference %zu bytes\n", lds, lds_judged,
           min_swap);
    return failed;
}

// the tables of gather_check mix: what they reach, and what their scatter inputs can tell
int mixed_selftest()
{
    int failed = 0;
    static const char *tn[3] = {"float16", "bfloat16", "float32"};
    auto need_t = [&](const char *what, int a, int b, size_t v) {
        if (v) return;
        failed++;
        if (b < 0) printf("FAIL the mixed tables never reach: %s (%s)\n", what, tn[a]);
        else printf("FAIL the mixed tables never reach: %s (%s, then %s)\n", what, tn[a], tn[b]);
    };
    // ---- coverage ----
    Cover X;
    MixCover M;
    const std::vector<Table> tabs = mix_tables();
    std::vector<std::vector<unsigned char>> paths;
    size_t pinned = 0, full = 0;
    for (const Table &T : tabs) {
        pinned += T.pinned;
        full += T.cnt.size() == (size_t)ftar::kMaxGather;
        const Layout L = layout(T);
        paths.emplace_back(T.elems(), 0);
        bool first = true;
        for (unsigned g : grids((unsigned)((L.total + kTile - 1) / kTile))) {
            failed += replay(T, g, X, first ? &paths.back() : nullptr, &M);
            first = false;
        }
    }
    printf("selftest: %zu mixed tables (%zu pinned, %zu of %d entries); each runs in both directions\n", tabs.size(), pinned, full,
           ftar::kMaxGather);
    printf("selftest: mixed: %zu pieces; workgroups with >= 2 tiles %zu; 2-byte groups: unrolled loop at 64 / 256 threads %zu / %zu, "
           "remainder %zu / %zu\n", X.pieces, X.wg_two_tiles, X.loops.unrolled[0], X.loops.unrolled[1], X.loops.rest[0], X.loops.rest[1]);
    for (int t = 0; t < 3; t++) {
        printf("selftest: mixed %s: the workgroup's pieces %zu, small on wave 0 / 1 / 2 / 3: %zu / %zu / %zu / %zu; tiles ending inside an "
               "entry %zu, at its end with %s / %s behind %zu / %zu; pieces in a workgroup's later tiles %zu; pieces of 1020 / 1024 / "
               "1028 bytes %zu / %zu / %zu\n", tn[t], M.big[t], M.small_wave[t][0], M.small_wave[t][1], M.small_wave[t][2],
               M.small_wave[t][3], M.inside[t], tn[(t + 1) % 3], tn[(t + 2) % 3], M.at_end[t][(t + 1) % 3], M.at_end[t][(t + 2) % 3],
               M.later_tile[t], M.threshold[t][0], M.threshold[t][1], M.threshold[t][2]);
        printf("selftest: mixed %s: in one tile behind float16 / bfloat16 / float32: %zu / %zu / %zu\n", tn[t], M.next_to[0][t],
               M.next_to[1][t], M.next_to[2][t]);
    }
    for (int t = 0; t < 2; t++)
        printf("selftest: mixed %s: class 8 / 4 / 2 with head, groups and tail: %zu / %zu / %zu, class 1: %zu\n", tn[t], M.cls_ht[t][0],
               M.cls_ht[t][1], M.cls_ht[t][2], M.cls_ht[t][3]);
    printf("selftest: mixed float32: vector pieces with body, tail and a head of 1 / 2 / 3 words: %zu / %zu / %zu, not vector %zu; "
           "unrolled loop at 256 threads %zu, remainder %zu; nvec = 1023 / 1024: %zu / %zu; word loops at 64 / 256 threads %zu / %zu\n",
           M.f_hbt[1], M.f_hbt[2], M.f_hbt[3], M.f_nonvec, M.f_loops.unrolled[1], M.f_loops.rest[1], M.f_loops.end_m1[1],
           M.f_loops.end_0[1], M.f_words[0], M.f_words[1]);
    failed += need("a pinned mixed table", pinned) + need("a mixed table of 1024 entries", full);
    for (int t = 0; t < 3; t++) {
        need_t("a piece of the workgroup", t, -1, M.big[t]);
        for (int w = 0; w < 4; w++) need_t("a small piece on each wave", t, -1, M.small_wave[t][w]);
        need_t("a tile ending inside an entry", t, -1, M.inside[t]);
        need_t("a piece in a workgroup's second tile or later", t, -1, M.later_tile[t]);
        static const char *thr[3] = {"a piece of 1020 packed bytes", "a piece of 1024 packed bytes", "a piece of 1028 packed bytes"};
        for (int k = 0; k < 3; k++) need_t(thr[k], t, -1, M.threshold[t][k]);
        for (int u = 0; u < 3; u++) {
            if (u != t) need_t("a tile ending at an entry's end with another type behind it", t, u, M.at_end[t][u]);
            need_t("two neighbours inside one tile", t, u, M.next_to[t][u]);
        }
    }
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 4; k++) need_t("every converting class with head and tail", t, -1, M.cls_ht[t][k]);
    for (int h = 1; h < 4; h++) failed += need("a float32 vector piece with body, tail and every head of 1, 2, 3 words", M.f_hbt[h]);
    failed += need("a float32 piece that is not a vector piece", M.f_nonvec) +
              need("float32: the unrolled loop at 256 threads", M.f_loops.unrolled[1]) + need("float32: its remainder", M.f_loops.rest[1]) +
              need("float32: nvec = 1023", M.f_loops.end_m1[1]) + need("float32: nvec = 1024", M.f_loops.end_0[1]) +
              need("float32: a word loop at 64 threads", M.f_words[0]) + need("float32: a word loop at 256 threads", M.f_words[1]);

    // ---- the gather inputs of the float32 entries: a signalling NaN as a word and inside a vector ----
    size_t snan[2] = {0, 0};
    for (size_t ti = 0; ti < tabs.size(); ti++) {
        const Table &T = tabs[ti];
        const Layout L = layout(T);
        for (size_t e = 0; e < T.cnt.size(); e++)
            if (!T.two_byte(e))
                for (size_t i = 0; i < T.cnt[e]; i++)
                    if (signalling(f32_user(T, e, i))) snan[paths[ti][L.first[e] + i] == 2]++;
    }
    failed += need("a signalling NaN gathered as a word", snan[0]) + need("a signalling NaN gathered in a 16-byte vector", snan[1]);

    // ---- the scatter inputs against the mutants, per case (table x scale) ----
    static const char *names[4] = {"rounding toward zero goes unseen", "ties away from zero go unseen",
                                   "flushed subnormal results go unseen", "a fused multiply-convert goes unseen"};
    size_t cases = 0, judged16 = 0, judged32 = 0, min_mut[4] = {SIZE_MAX, SIZE_MAX, SIZE_MAX, SIZE_MAX}, upper_half = 0;
    size_t neg_zero[2][2] = {{0, 0}, {0, 0}};                                 // 2-byte: [type][alone, in a group]
    size_t min_flush = SIZE_MAX, min_unscaled = SIZE_MAX;                     // float32, per case
    size_t flush_at[2] = {0, 0}, unscaled_at[2] = {0, 0}, zero_at[2] = {0, 0}; // float32, over the matrix: [word, vector]
    double max_nan = 0, min_finite = 1;
    for (size_t ti = 0; ti < tabs.size(); ti++) {
        const Table &T = tabs[ti];
        const Layout L = layout(T);
        const size_t n = T.elems();
        for (float scale : kScales) {
            cases++;
            size_t nan = 0, fin = 0, mut[4] = {0, 0, 0, 0}, flush = 0, unscaled = 0;
            for (size_t e = 0; e < T.cnt.size(); e++)
                for (size_t i = 0; i < T.cnt[e]; i++) {
                    const size_t g = L.sub[e] + i;
                    const int way = paths[ti][L.first[e] + i] == 2;
                    if (T.two_byte(e)) {
                        const int dt = T.ty[e];
                        const float a = cvt_packed(T, dt, scale, g);
                        const uint16_t w = narrow_ref(a, scale, dt);
                        const double v = decode16(w, dt);
                        nan += std::isnan(v);
                        fin += std::isfinite(v) && v != 0.0;
                        if (std::isnan(v)) {
                            upper_half += !is_nan16(narrow_ref(a, scale, dt, kUpperHalf), dt);
                            continue;
                        }
                        for (int m = 0; m < 4; m++) mut[m] += narrow_ref(a, scale, dt, m + 1) != w;
                        if (scale != 0.0f && w == 0x8000) neg_zero[dt == kBFloat16][way]++;
                    } else {
                        const float a = f32_packed(T, scale, g);
                        const uint32_t w = scale_ref(a, scale);
                        const float v = f32_of(w);
                        nan += std::isnan(v);
                        fin += std::isfinite(v) && v != 0.0f;
                        if (std::isnan(v) || scale == 0.0f) continue; // NaN: compared by NaN-ness, every mutant gives one as well
                        const bool f = scale_ref(a, scale, kFlushProduct) != w, u = scale_ref(a, scale, kNotScaled) != w;
                        flush += f;
                        unscaled += u;
                        flush_at[way] += f;
                        unscaled_at[way] += u;
                        zero_at[way] += scale_ref(a, scale, kPlusZero) != w;
                    }
                }
            const double sn = (double)nan / (double)n, sf = (double)fin / (double)n;
            auto bad = [&](const char *why) {
                failed++;
                printf("FAIL %s scale %.9g: %s\n", T.name.c_str(), scale, why);
            };
            if (T.block != kNonFinite) {
                if (sn > max_nan) max_nan = sn;
                if (nan * 8 > n) bad("more than 1/8 of the expected elements are NaN");
            }
            if (scale == 0.0f) continue;
            if (n >= 257) {
                if (sf < min_finite) min_finite = sf;
                if (fin * 2 < n) bad("fewer than half of the expected elements are finite and non-zero");
            }
            if (L.n16 >= 257) {
                judged16++;
                for (int m = 0; m < 4; m++) {
                    if (m == 3 && exact_scale(scale)) continue;
                    if (mut[m] < min_mut[m]) min_mut[m] = mut[m];
                    if (!mut[m]) bad(names[m]);
                }
            }
            if (L.n32 >= 257) {
                judged32++;
                if (flush < min_flush) min_flush = flush;
                if (!flush) bad("a float32 subnormal product flushed to zero goes unseen");
                if (scale != 1.0f) {
                    if (unscaled < min_unscaled) min_unscaled = unscaled;
                    if (!unscaled) bad("a float32 entry that is not scaled goes unseen");
                }
            }
        }
    }
    printf("selftest: %zu mixed scatter cases at a scale other than 0: %zu with >= 257 2-byte elements, %zu with >= 257 float32 elements\n",
           cases - tabs.size(), judged16, judged32);
    printf("selftest: mixed: largest NaN share %.4f, smallest finite non-zero share %.4f\n", max_nan, min_finite);
    printf("selftest: mixed 2-byte: smallest mutant difference (elements): toward zero %zu, ties away %zu, subnormals flushed %zu, fused "
           "%zu; an infinity for a NaN seen in %zu; -0 expected alone / in a group: float16 %zu / %zu, bfloat16 %zu / %zu\n", min_mut[0],
           min_mut[1], min_mut[2], min_mut[3], upper_half, neg_zero[0][0], neg_zero[0][1], neg_zero[1][0], neg_zero[1][1]);
    printf("selftest: mixed float32: smallest mutant difference (elements): subnormal product flushed %zu, not scaled %zu; seen in a word "
           "/ in a 16-byte vector: flushed %zu / %zu, not scaled %zu / %zu, +0 for a -0 product %zu / %zu; signalling NaNs to gather "
           "%zu / %zu\n", min_flush, min_unscaled, flush_at[0], flush_at[1], unscaled_at[0], unscaled_at[1], zero_at[0], zero_at[1],
           snan[0], snan[1]);
    failed += need("a NaN whose upper half reads as an infinity, in a mixed table", upper_half);
    for (int t = 0; t < 2; t++)
        failed += need("mixed: -0 in an element that moves alone", neg_zero[t][0]) + need("mixed: -0 in an element of a group", neg_zero[t][1]);
    for (int w = 0; w < 2; w++)
        failed += need(w ? "a flushed float32 product in a 16-byte vector" : "a flushed float32 product in a word", flush_at[w]) +
                  need(w ? "an unscaled float32 element in a 16-byte vector" : "an unscaled float32 element in a word", unscaled_at[w]) +
                  need(w ? "a float32 -0 product in a 16-byte vector" : "a float32 -0 product in a word", zero_at[w]);
    return failed;
}

} // namespace

static int selftest()
{
    Stats S;
    std::set<std::tuple<int, int, int, size_t, uint64_t>> seen; // variants of a case share their inputs
    size_t ntree = 0, nbatch = 0, npiece = 0;
    for (const TreeCase &c : tree_cases()) {
        ntree++;
        if (seen.insert(std::make_tuple(c.dt, c.op, c.p, c.n, c.seed)).second) judge(S, "tree", c.dt, c.op, c.p, c.n, c.seed);
    }
    for (const BatchCase &c : batch_cases())
        for (int k = 0; k < c.ntree; k++) {
            nbatch++;
            judge(S, "batch tree", c.dt, c.op, c.p, c.tree_n(k), c.tree_seed(k));
        }
    for (int li = 0; li < kSegLists; li++) {
        const SegList L = seg_list(li);
        for (const SegPiece &P : L.pc)
            if (P.kind == 1) {
                npiece++;
                judge(S, "piece", L.dt, L.op, 2, P.n, P.seed);
            }
    }
    printf("selftest: %zu tree cases, %zu batch trees, %zu reduce pieces: %d distinct inputs, %d of n >= 257\n", ntree, nbatch,
           npiece, S.cases, S.judged);
    printf("selftest: largest NaN share %.4f, smallest finite non-zero share %.4f\n", S.max_nan, S.min_finite);
    printf("selftest: smallest mutant difference (elements): toward zero %zu, ties away %zu, subnormals flushed %zu\n",
           S.min_mut[0], S.min_mut[1], S.min_mut[2]);
    printf("selftest: smallest swap difference %zu bytes (FTAR_2INT: largest %zu)\n", S.min_swap, S.max_swap_2int);
    S.failed += movers_selftest();
    S.failed += mixed_selftest();
    printf("selftest: %d failed\n", S.failed);
    return S.failed ? 1 : 0;
}

static int narrow(int dt, const char *fin, const char *fout)
{
    const Bytes in = read_file(fin);
    if (!is16(dt) || in.size() % 4) {
        fprintf(stderr, "ref_check: narrow wants dtype 16 or 17 and a file of float32\n");
        return 2;
    }
    std::vector<uint16_t> out(in.size() / 4);
    for (size_t i = 0; i < out.size(); i++) {
        float a;
        memcpy(&a, &in[4 * i], 4);
        out[i] = kmov::narrow_ref(a, 1.0f, dt);
    }
    FILE *f = fopen(fout, "wb");
    if (!f || fwrite(out.data(), 2, out.size(), f) != out.size()) {
        perror(fout);
        return 2;
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "apply")) return apply(atoi(argv[2]), atoi(argv[3]), argv[4], argv[5], argv[6]);
    if (argc == 2 && !strcmp(argv[1], "selftest")) return selftest();
    if (argc == 5 && !strcmp(argv[1], "narrow")) return narrow(atoi(argv[2]), argv[3], argv[4]);
    fprintf(stderr, "usage: ref_check apply DTYPE OP IN INOUT OUT | ref_check selftest | ref_check narrow DTYPE IN OUT\n");
    return 2;
}
