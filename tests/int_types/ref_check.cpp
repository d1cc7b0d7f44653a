// TEST-ONLY host program (no HIP call, no GPU): the reference of int_ref.h on operand files, the
// self-test of the GPU checker's inputs, and a walk of the gather mover's pieces at 1- and 2-byte
// elements (gather_piece is ftar_kernels.h's own: nothing of the product is linked).  Built plain
// and with ASan + UBSan (Makefile).  The planners' walk at these sizes: tests/kernel_plan.
//
//   ref_check apply <dtype> <op> <in file> <inout file> <out file>
//       out = inout op in, element by element (raw little-endian files of equal size)
//   ref_check selftest
//       for every (type, op) and every case length of int_check: the generated operands give a
//       different result under each wrong kernel of int_ref.h that applies to the op; the canonical
//       dispatch (ftar::canon_dtype) names a type of the same width whose reference result is the
//       same bytes on those operands and on a sweep of specials
//   ref_check planwalk
//       gather_piece at esize 1 and 2: every start offset 0..15 bytes the alignment allows (user and
//       packed side co-aligned or not), every length 0..64 and one past a full 16 KiB tile: every
//       byte moved exactly once, no access misaligned to its unit, vector accesses 16-byte aligned
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

// ---- gather walk ----------------------------------------------------------------------------
static size_t ES;

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
        std::vector<size_t> sizes;
        for (size_t n = 0; n <= 64; n++) sizes.push_back(n);
        sizes.push_back((16384 + 16) / es + 3);
        for (size_t n : sizes)
            for (unsigned mo = 0; mo < 16; mo += (unsigned)es)
                for (unsigned mx = 0; mx < 16; mx += (unsigned)es) {
                    if (mx != mo && n > 64 && (mo + mx) % 5) continue; // all scalar there: a few pairs
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
