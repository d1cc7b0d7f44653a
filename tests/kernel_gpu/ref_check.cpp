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
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

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
    printf("selftest: %d failed\n", S.failed);
    return S.failed ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "apply")) return apply(atoi(argv[2]), atoi(argv[3]), argv[4], argv[5], argv[6]);
    if (argc == 2 && !strcmp(argv[1], "selftest")) return selftest();
    fprintf(stderr, "usage: ref_check apply DTYPE OP IN INOUT OUT | ref_check selftest\n");
    return 2;
}
