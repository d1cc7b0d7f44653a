// TEST-ONLY host program (no HIP call, no GPU): the reference of int_ref.h on operand files, the
// self-test of the GPU checker's inputs, and a walk of the four planners at 1- and 2-byte
// elements.  Built plain and with ASan + UBSan (Makefile); the planners themselves come from the
// product's kernel object, their index arithmetic is replayed here.
//
//   ref_check apply <dtype> <op> <in file> <inout file> <out file>
//       out = inout op in, element by element (raw little-endian files of equal size)
//   ref_check selftest
//       for every (type, op) and every case length of int_check: the generated operands give a
//       different result under each wrong kernel of int_ref.h that applies to the op; the canonical
//       dispatch (ftar::canon_dtype) names a type of the same width whose reference result is the
//       same bytes on those operands and on a sweep of specials
//   ref_check planwalk
//       plan_segments, plan_tree, plan_tree_batch and gather_piece at esize 1 and 2: every start
//       offset 0..15 bytes the alignment allows (sources co-aligned or not), every length 0..64 and
//       one past a full 16 KiB tile: every element covered exactly once, no access misaligned to
//       its width, vector accesses 16-byte aligned
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../fault-tolerant_amd/csrc/ftar_kernels.h"
#include "int_ref.h"

using namespace ftar;

static_assert(iref::kInt8 == ftar::kInt8 && iref::kUInt8 == ftar::kUInt8 && iref::kInt16 == ftar::kInt16 &&
                  iref::kUInt16 == ftar::kUInt16 && iref::kUInt32 == ftar::kUInt32 && iref::kUInt64 == ftar::kUInt64 &&
                  iref::kSum == ftar::kSum && iref::kBxor == ftar::kBxor && iref::kNumOps == ftar::kNumOps,
              "the reference's numbers are the product's");

static bool read_file(const char *path, iref::Bytes *b)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    b->resize(n > 0 ? (size_t)n : 0);
    const bool ok = n >= 0 && fread(b->data(), 1, b->size(), f) == b->size();
    fclose(f);
    return ok;
}

static int cmd_apply(char **a)
{
    const int dt = atoi(a[0]), op = atoi(a[1]);
    const size_t es = iref::esize(dt);
    iref::Bytes in, io;
    if (!es || op < 0 || op >= iref::kNumOps || !read_file(a[2], &in) || !read_file(a[3], &io) || in.size() != io.size() ||
        in.size() % es) {
        fprintf(stderr, "apply: bad arguments\n");
        return 2;
    }
    iref::reduce_local(dt, op, in.data(), io.data(), io.size() / es);
    FILE *f = fopen(a[4], "wb");
    if (!f || fwrite(io.data(), 1, io.size(), f) != io.size()) return 2;
    fclose(f);
    return 0;
}

// the width's canonical type: the int32 / int64 of the product are not in int_ref.h's list, so
// they are modelled by the unsigned type of the same width (identical bits but for MAX / MIN,
// which canon_dtype never sends there)
static int model_of(int canon)
{
    if (canon == ftar::kInt32) return iref::kUInt32;
    if (canon == ftar::kInt64) return iref::kUInt64;
    return canon;
}

static int cmd_selftest()
{
    long checks = 0;
    for (int dt : iref::kTypes)
        for (int op = 0; op < iref::kNumOps; op++) {
            const size_t es = iref::esize(dt);
            const int canon = canon_dtype(dt, op), model = model_of(canon);
            if (iref::esize(model) != es) {
                fprintf(stderr, "canon_dtype(%d, %d) = %d crosses widths\n", dt, op, canon);
                return 1;
            }
            if ((op == iref::kMax || op == iref::kMin) && canon != dt) {
                fprintf(stderr, "canon_dtype(%d, %d) = %d: MAX / MIN need the type's own signedness\n", dt, op, canon);
                return 1;
            }
            for (size_t n : iref::case_lengths(es)) {
                iref::Bytes x(n * es), y(n * es);
                iref::fill(dt, op, n, 0, iref::case_seed(dt, op, n), x.data());
                iref::fill(dt, op, n, 1, iref::case_seed(dt, op, n), y.data());
                iref::Bytes want = x, viacanon = x;
                iref::reduce_local(dt, op, y.data(), want.data(), n);
                iref::reduce_local(model, op, y.data(), viacanon.data(), n);
                if (want != viacanon) {
                    fprintf(stderr, "dtype %d op %d: the canonical type %d computes other bits\n", dt, op, canon);
                    return 1;
                }
                for (int m = 0; m < iref::kNumMutants; m++) {
                    if (!iref::applies(m, dt, op)) continue;
                    iref::Bytes got = x;
                    iref::mutant_reduce(m, dt, op, y.data(), got.data(), n);
                    checks++;
                    if (got == want) {
                        fprintf(stderr, "dtype %d op %d, %zu elements: the inputs do not expose %s\n", dt, op, n, iref::mutant_name(m));
                        return 1;
                    }
                }
            }
        }
    printf("selftest OK %ld wrong kernels exposed\n", checks);
    return 0;
}

// ---- planner walk ---------------------------------------------------------------------------
static size_t ES, EPV;

static int fail(const char *what, size_t n, unsigned mo, unsigned mx)
{
    fprintf(stderr, "esize %zu, n %zu, out at byte %u, source at byte %u: %s\n", ES, n, mo, mx, what);
    return 1;
}
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

// mo, mx: byte offsets (multiples of ES) of the output / own operand and of the other source
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
        if (off < 0 || off % (intptr_t)ES || (intptr_t)S.x - (intptr_t)in.x != off) return fail("segments: piece offsets", n, mo, mx);
        if (((uintptr_t)S.out | (uintptr_t)S.x | (uintptr_t)S.y | (uintptr_t)S.out2) % ES)
            return fail("segments: an access misaligned to the element", n, mo, mx);
        const size_t e0 = (size_t)off / ES;
        if (S.vec) {
            any_vec = true;
            if ((((uintptr_t)S.out | (uintptr_t)S.x | (uintptr_t)S.y | (uintptr_t)S.out2) & 15) || S.n % EPV)
                return fail("segments: vector piece not 16-byte aligned", n, mo, mx);
            const size_t nv = S.n / EPV;
            for (size_t t = w.first; t * kTileVecs < nv; t += w.stride)
                for (size_t v = t * kTileVecs; v < nv && v < (t + 1) * kTileVecs; v++)
                    for (size_t k = 0; k < EPV; k++)
                        if (!hit(cnt, e0 + v * EPV + k)) return fail("segments: vector past the end", n, mo, mx);
        } else {
            if (S.n >= 2 * EPV && mo == mx) return fail("segments: a scalar piece of a vector's length and more", n, mo, mx);
            for (size_t s = w.first; s * 256 < S.n; s += w.stride)
                for (size_t i = s * 256; i < S.n && i < (s + 1) * 256; i++)
                    if (!hit(cnt, e0 + i)) return fail("segments: element past the end", n, mo, mx);
        }
    }
    if (!once(cnt)) return fail("segments: an element not written exactly once", n, mo, mx);
    if (mo == mx && n >= 2 * EPV && !any_vec) return fail("segments: co-aligned operands without a vector body", n, mo, mx);
    if (mo != mx && any_vec) return fail("segments: a vector body on operands that are not co-aligned", n, mo, mx);
    return 0;
}

static int walk_tree(const TreeArgs &A, int p, unsigned nblocks, size_t n, unsigned mo, unsigned mx)
{
    const unsigned U = A.unroll;
    std::vector<uint8_t> cnt(n, 0);
    for (int j = 0; j < p; j++)
        if ((uintptr_t)A.src[j] % ES) return fail("tree: a source misaligned to the element", n, mo, mx);
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
    if (!once(cnt)) return fail("tree: an element not written exactly once", n, mo, mx);
    if (mo == mx && n >= 2 * EPV && !A.nv) return fail("tree: co-aligned sources without a vector body", n, mo, mx);
    if (mo != mx && A.nv) return fail("tree: a vector body on sources that are not co-aligned", n, mo, mx);
    return 0;
}

static void fill_tree(TreeArgs *A, int p, size_t n, unsigned mo, unsigned mx, unsigned unroll, int nmore, int slot)
{
    const uintptr_t base = (uintptr_t)(slot + 1) << 44;
    *A = TreeArgs{};
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

// p trees over consecutive windows of one vector: Raben's blocks, which at 1-byte elements begin
// on odd BYTE addresses
static int check_batch(int p, size_t n, unsigned mo, unsigned mx, unsigned cap)
{
    TreeBatch B;
    B.nt = 0;
    B.sig = KSignal{};
    std::vector<size_t> len;
    std::vector<unsigned> tmo, tmx;
    size_t at = 0;
    for (int k = 0; k < p; k++) {
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

// One entry of n elements at user byte offset mu, packed at byte offset mp of a packed vector that
// begins 16-byte aligned; the tiles of the packed vector walked as gather_kernel walks them and
// every piece moved as move_piece moves it.
static int check_gather(size_t n, unsigned mu, unsigned mp)
{
    if (n == 0) return 0; // the table holds no empty entry
    const uintptr_t user = ((uintptr_t)5 << 40) + mu;
    const char *packed = (const char *)((uintptr_t)6 << 40);
    const GEntry tab[2] = {{(void *)((uintptr_t)7 << 40), 0, mp}, {(void *)user, mp, n * ES}};
    const GEntry *t0 = mp ? tab : tab + 1; // (a filler entry in front puts the entry at packed byte mp)
    const int nt = mp ? 2 : 1;
    const size_t total = mp + n * ES;
    std::vector<uint8_t> cnt(n * ES, 0);
    auto units = [&](uintptr_t u, uintptr_t k, size_t bytes, unsigned unit) {
        if (bytes % unit || u % unit || k % unit) return false;
        for (size_t b = 0; b < bytes; b++)
            if (!hit(cnt, (size_t)(u - user) + b)) return false;
        return true;
    };
    for (size_t lo = 0; lo < total; lo += kTileBytes) {
        const size_t hi = lo + kTileBytes < total ? lo + kTileBytes : total;
        for (int e = gather_first(t0, nt, lo); e < nt; e++) {
            GPiece P;
            if (!gather_piece(t0[e], lo, hi, packed, (unsigned)ES, &P)) break;
            if (t0[e].ptr != (void *)user) continue; // the filler
            const uintptr_t u = (uintptr_t)P.user, k = (uintptr_t)packed + P.poff;
            if (P.unit != ES && !(P.unit < ES)) return fail("gather: a unit wider than the element", n, mu, mp);
            if (ES % P.unit) return fail("gather: a unit that does not divide the element", n, mu, mp);
            if (u - user != P.poff - mp) return fail("gather: user and packed offsets apart", n, mu, mp);
            if (!units(u, k, P.head, P.unit)) return fail("gather: head misaligned to its unit or outside", n, mu, mp);
            if (P.vec) {
                if (((u + P.head) | (k + P.head)) & 15 && P.nvec) return fail("gather: vectors misaligned", n, mu, mp);
                if (P.head >= 16 && P.head != P.bytes) return fail("gather: a head of a vector's length", n, mu, mp);
                if (!units(u + P.head, k + P.head, P.nvec * 16, 1)) return fail("gather: vector outside", n, mu, mp);
                const size_t done = P.head + P.nvec * 16;
                if (P.bytes - done >= 16) return fail("gather: a tail of a vector's length", n, mu, mp);
                if (!units(u + done, k + done, P.bytes - done, P.unit)) return fail("gather: tail misaligned to its unit", n, mu, mp);
            } else if (P.head != P.bytes || P.nvec) {
                return fail("gather: an unaligned piece with a vector body", n, mu, mp);
            }
            if ((mu % 16 == mp % 16) != (P.vec != 0)) return fail("gather: vec does not follow co-alignment", n, mu, mp);
        }
    }
    if (!once(cnt)) return fail("gather: a byte not moved exactly once", n, mu, mp);
    return 0;
}

static int cmd_planwalk()
{
    long cases = 0;
    for (size_t es : {(size_t)1, (size_t)2}) {
        ES = es;
        EPV = 16 / es;
        std::vector<size_t> sizes;
        for (size_t n = 0; n <= 64; n++) sizes.push_back(n);
        sizes.push_back((16384 + 16) / es + 3);
        for (size_t n : sizes)
            for (unsigned mo = 0; mo < 16; mo += (unsigned)es)
                for (unsigned mx = 0; mx < 16; mx += (unsigned)es) {
                    if (mx != mo && n > 64 && (mo + mx) % 5) continue; // all scalar there: a few pairs
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
                    if (check_gather(n, mo, mx)) return 1;
                    cases++;
                }
    }
    printf("planwalk OK %ld cases\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "apply")) return cmd_apply(argv + 2);
    if (argc == 2 && !strcmp(argv[1], "selftest")) return cmd_selftest();
    if (argc == 2 && !strcmp(argv[1], "planwalk")) return cmd_planwalk();
    fprintf(stderr, "usage: ref_check apply <dtype> <op> <in> <inout> <out> | selftest | planwalk\n");
    return 2;
}
