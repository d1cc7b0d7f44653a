// TEST-ONLY, host-only: the inputs and the case lists of tree_check's and seg_check's `types`
// matrices (float16 / bfloat16 x SUM, PROD, MAX, MIN; the three pair types x MAXLOC, MINLOC),
// shared with ref_check, whose selftest asserts on the CPU that these inputs can tell a wrong
// kernel from a right one (tests/test_kernel_ref.py).
//
// Every value is a function of (seed, source, element): no generator state, so the checkers and
// the selftest see the same bytes.  SUM / PROD fills are random values that round (SUM: 2^-10 ..
// 2^11, sixteen of them stay finite in binary16; PROD: +-(1 + k ulp), k < 8) with one element in
// eight CONSTRUCTED: two of the p sources carry a pair of operands and every other source the
// identity (+0, 1), so the pair meets once, in whichever level of the tree joins the two -- exact
// ties on even and odd neighbours, sums and products that land in the subnormal range, on a tie
// there too, cancellation, overflow and the overflowing tie at the largest finite value; and at
// a fixed sparse set of positions infinities (inf + x, inf - inf).  MAX / MIN fills carry NaNs
// of both signs and many payloads, +-0 and infinities; pair fills values from a small set (ties),
// +-0, NaN, infinities, indices from a small range and random padding, so elements equal in
// value and index whose bytes differ occur (FTAR_2INT has no such elements: its bytes ARE value
// and index, and its result does not depend on the operand order at all).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ref_types.h"

namespace kgen {
using namespace kref;

struct Combo { int dt, op; };
static const Combo kCombos[14] = {
    {kFloat16, kSum},  {kFloat16, kProd},  {kFloat16, kMax},  {kFloat16, kMin},  {kBFloat16, kSum},
    {kBFloat16, kProd}, {kBFloat16, kMax}, {kBFloat16, kMin}, {kFloatInt, kMaxloc}, {kFloatInt, kMinloc},
    {k2Int, kMaxloc},  {k2Int, kMinloc},   {kDoubleInt, kMaxloc}, {kDoubleInt, kMinloc}};

inline bool rounds(const Combo &c) { return is16(c.dt) && (c.op == kSum || c.op == kProd); }
// the result depends on which operand is x: compare-and-select with NaN, +-0 or padding to tell
inline bool order_sensitive(const Combo &c) { return (is16(c.dt) && !rounds(c)) || c.dt == kFloatInt || c.dt == kDoubleInt; }

inline uint64_t mix(uint64_t x)
{
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// ---- 16-bit patterns by their fields -------------------------------------------------
struct F16 {
    int mb, bias, emax, emin;
    unsigned mask;
    explicit F16(int dt) : mb(mant_bits(dt)), bias((1 << (exp_bits(dt) - 1)) - 1), emax(bias), emin(1 - bias), mask((1u << mb) - 1) {}
    uint16_t mk(unsigned s, int e, unsigned m) const { return (uint16_t)((s & 1) << 15 | (unsigned)(e + bias) << mb | (m & mask)); }
    uint16_t sub(unsigned s, unsigned m) const { return (uint16_t)((s & 1) << 15 | (m & mask)); }
    uint16_t inf(unsigned s) const { return mk(s, emax + 1, 0); }
    uint16_t nan(unsigned s, unsigned m) const { return mk(s, emax + 1, (m & mask) ? m : 1); }
};

inline uint16_t value16(int dt, int op, size_t i, int j, int p, uint64_t seed)
{
    const F16 f(dt);
    const uint64_t hp = mix(seed ^ mix(i)), he = mix(hp ^ mix((uint64_t)j + 1));
    const unsigned s = (unsigned)(he >> 4) & 1, m = (unsigned)(he >> 16) & f.mask;
    if (op == kMax || op == kMin) {
        switch (he % 16) {
        case 0: return f.sub(0, 0);
        case 1: return f.sub(1, 0);
        case 2: return f.nan(s, m);
        case 3: return f.nan(s, 1u << (f.mb - 1) | m);
        case 4: return f.inf(0);
        case 5: return f.inf(1);
        case 6: return f.mk(s, (int)((hp >> 8) % 3), (unsigned)(hp >> 16) & 3); // a few values, the same on many sources: ties
        default: {
            uint16_t b = (uint16_t)(he >> 32);
            if ((b & f.inf(0)) == f.inf(0)) b &= 0xBFFF; // finite
            return b;
        }
        }
    }
    const uint16_t ident = op == kSum ? f.sub(0, 0) : f.mk(0, 0, 0);
    const int a = (int)((hp >> 8) % (unsigned)p), b = (a + 1 + (int)((hp >> 16) % (unsigned)(p - 1))) % p; // b != a
    const unsigned r = (unsigned)(hp >> 24), sa = r & 1, sb = (r >> 1) & 1, ma = (r >> 4) & f.mask, mb2 = (r >> 14) & f.mask;
    if (i % 509 == 100) { // the fixed sparse set: an infinity and a finite value, or two opposed infinities (NaN)
        if (j == a) return f.inf(sa);
        if (j == b) return i % 1018 == 100 ? (op == kSum ? f.inf(!sa) : f.sub(sb, 0)) : f.mk(sb, 0, ma);
        return ident;
    }
    if ((hp & 7) == 0) { // constructed: sources a and b carry the operands, the others the identity
        if (j != a && j != b) return ident;
        const bool A = j == a;
        if (op == kSum) {
            switch ((hp >> 3) % 6) {
            case 0: { // an exact tie: a value and half its ulp
                const int e = (int)((r >> 24) % 9);
                return A ? f.mk(sa, e, ma) : f.mk(sa, e - f.mb - 1, 0);
            }
            case 1: return A ? f.sub(sa, 1 + ma % ((1u << (f.mb - 1)) - 1)) : f.sub(sa, 1 + mb2 % ((1u << (f.mb - 1)) - 1)); // subnormal sum
            case 2: return A ? f.mk(sa, f.emin, ma) : f.mk(!sa, f.emin, mb2); // cancels into the subnormal range
            case 3: { // cancels to +0, or to one ulp
                const int e = (int)((r >> 24) % 21) - 10;
                return A ? f.mk(sa, e, ma) : f.mk(!sa, e, ma ^ (sb & 1));
            }
            case 4: return A ? f.mk(sa, f.emax, ma | 1u << (f.mb - 1)) : f.mk(sa, f.emax, mb2); // overflows
            default: return A ? f.mk(sa, f.emax, f.mask) : f.mk(sa, f.emax - f.mb - 1, 0); // the largest finite value and half its ulp
            }
        }
        switch ((hp >> 3) % 5) {
        case 0: return A ? f.mk(sa, 0, (ma % 32) | 1) : f.mk(sb, 0, 1u << (f.mb - 1)); // (1 + m ulp) * 1.5, m odd: a tie
        case 1: return A ? ((r >> 24) & 1 ? f.mk(sa, f.emin, ma) : f.sub(sa, ma | 1)) : f.mk(sb, -1, 0); // halved into a subnormal, a tie if odd
        case 2: return A ? f.mk(sa, f.emin + 2, ma) : f.mk(sb, -5, mb2); // a subnormal product that rounds
        case 3: return A ? f.mk(sa, f.emax, ma) : f.mk(sb, 1, mb2); // overflows
        default: return A ? f.mk(sa, (int)((r >> 24) % 21) - 10, ma) : f.sub(sb, 0); // a signed zero
        }
    }
    if (op == kProd) return f.mk(s, 0, (unsigned)(he >> 8) % 8); // +-(1 + k ulp): ulp = 1/1024 (float16), 1/128 (bfloat16)
    switch (he % 16) {
    case 0: return f.sub(0, 0);
    case 1: return f.sub(1, 0);
    case 2: return f.sub(s, m);
    default: return f.mk(s, (int)((he >> 8) % 21) - 10, m); // 2^-10 .. 2^11
    }
}

inline void value_pair(unsigned char *e, int dt, size_t i, int j, uint64_t seed)
{
    const uint64_t hp = mix(seed ^ mix(i)), he = mix(hp ^ mix((uint64_t)j + 1)), h2 = mix(he);
    const unsigned c = (unsigned)(he % 16);
    // indices from a small range, on one element in four the same on every source
    int32_t idx = (int32_t)((he >> 8) % 4) - 2;
    if ((hp & 3) == 0) idx = (int32_t)((hp >> 8) % 4) - 2;
    if ((he >> 12) % 32 == 0) idx = (he >> 20) & 1 ? INT32_MAX : INT32_MIN;
    if (dt == k2Int) {
        int32_t v = (int32_t)(h2 >> 16);
        if (c < 10) v = (int32_t)(c % 5) - 2;
        else if (c == 15) v = (h2 & 1) ? INT32_MAX : INT32_MIN;
        memcpy(e, &v, 4);
        memcpy(e + 4, &idx, 4);
        return;
    }
    static const double few[] = {-1.0, 0.5, 1.0, 2.0, -0.0, 0.0};
    double v = ((double)(int64_t)((h2 >> 20) % 2001) - 1000.0) / (double)(1 << ((h2 >> 40) % 6));
    uint64_t nanbits = 0x7ff8000000000000ull | ((uint64_t)(h2 & 1) << 63);
    if (c == 0) v = 0.0;
    else if (c == 1) v = -0.0;
    else if (c == 2) memcpy(&v, &nanbits, 8);
    else if (c == 3) v = 1.0 / 0.0;
    else if (c == 4) v = -1.0 / 0.0;
    else if (c < 11) v = few[c - 5];
    if (dt == kFloatInt) {
        const float fv = (float)v;
        memcpy(e, &fv, 4);
        memcpy(e + 4, &idx, 4);
    } else {
        const uint32_t pad = (uint32_t)(h2 >> 8);
        memcpy(e, &v, 8);
        memcpy(e + 8, &idx, 4);
        memcpy(e + 12, &pad, 4);
    }
}

// source j of p (a segment's x is source 0, its y source 1), n elements
inline void fill(unsigned char *buf, int dt, int op, size_t n, int j, int p, uint64_t seed)
{
    if (is16(dt)) {
        for (size_t i = 0; i < n; i++) {
            const uint16_t v = value16(dt, op, i, j, p, seed);
            memcpy(buf + 2 * i, &v, 2);
        }
    } else {
        const size_t es = esize(dt);
        for (size_t i = 0; i < n; i++) value_pair(buf + i * es, dt, i, j, seed);
    }
}

typedef std::vector<unsigned char> Bytes;

inline std::vector<Bytes> sources(int dt, int op, size_t n, int p, uint64_t seed)
{
    std::vector<Bytes> src(p, Bytes(n * esize(dt)));
    for (int j = 0; j < p; j++) fill(src[j].data(), dt, op, n, j, p, seed);
    return src;
}

// the balanced left-to-right tree over src[0..p-1], every combination by the reference
// (inout = inout op in); `swapped`: the operands of every combination exchanged
inline Bytes tree_expect(const std::vector<Bytes> &src, int p, int dt, int op, size_t n, bool swapped,
                         Round mode = kNearestEven)
{
    std::vector<Bytes> v(src.begin(), src.begin() + p);
    for (int w = 1; w < p; w *= 2)
        for (int j = 0; j < p; j += 2 * w) {
            const int a = swapped ? j + w : j, b = swapped ? j : j + w;
            if (reduce_local(dt, op, v[b].data(), v[a].data(), n, mode) != 0) {
                fprintf(stderr, "reference refused dtype %d op %d\n", dt, op);
                exit(2);
            }
            if (swapped) v[j].swap(v[j + w]);
        }
    return v[0];
}

// elements that differ; a 16-bit SUM / PROD element whose expectation is a NaN counts only if
// the other side is not one (NaN-ness: the payload of an arithmetic NaN is not specified)
inline size_t count_diff(const unsigned char *got, const unsigned char *want, int dt, int op, size_t n, size_t *first = nullptr)
{
    const size_t es = esize(dt);
    const bool nanness = is16(dt) && (op == kSum || op == kProd);
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        bool same = !memcmp(got + i * es, want + i * es, es);
        if (!same && nanness) {
            uint16_t g, w;
            memcpy(&g, got + 2 * i, 2);
            memcpy(&w, want + 2 * i, 2);
            same = is_nan16(w, dt) && is_nan16(g, dt);
        }
        if (!same && !bad++ && first) *first = i;
    }
    return bad;
}

// ---- windows: byte offsets past a 16-byte boundary -------------------------------------
// 2-byte: heads of 7, 5 and 1 elements; 8-byte pairs: 8 is a head of one element, 4 and 12 the
// scalar path although co-aligned; the 16-byte pair: 8 is the scalar path
inline const std::vector<int> &offsets(size_t es)
{
    static const std::vector<int> o2 = {0, 2, 6, 14}, o8 = {0, 8, 4, 12}, o16 = {0, 8};
    return es == 2 ? o2 : es == 8 ? o8 : o16;
}
inline const std::vector<size_t> &lengths(size_t es)
{
    static const std::vector<size_t> l2 = {1, 7, 8, 9, 263, 4099, (1u << 16) + 11}, l8 = {1, 2, 3, 257, 4099, (1u << 15) + 5},
                                     l16 = {1, 2, 257, 4099, (1u << 14) + 3};
    return es == 2 ? l2 : es == 8 ? l8 : l16;
}

// ---- tree_kernel cases -------------------------------------------------------------------
struct TreeCase {
    int dt, op, p, unroll;
    size_t n;
    int off; // >= 0: every pointer at this byte offset past a 16-byte boundary; -1: pointer k at offsets[k % size]
    int nmore;
    unsigned nt;
    uint64_t seed; // of the inputs: a function of (dt, op, p, n) -- the unroll / window / store variants share them
    size_t ptr_off(int k) const
    {
        const std::vector<int> &o = offsets(esize(dt));
        return off >= 0 ? (size_t)off : (size_t)o[(size_t)k % o.size()];
    }
};

inline std::vector<TreeCase> tree_cases()
{
    std::vector<TreeCase> out;
    for (const Combo &c : kCombos) {
        const size_t es = esize(c.dt);
        const std::vector<int> &offs = offsets(es);
        for (int p : {2, 4, 8, 16})
            for (int u : {1, 2, 4}) {
                if (u > 1 && p != 4 && p != 8) continue; // unrolled forms exist at p = 4, 8 only
                unsigned k = 0;
                for (size_t n : lengths(es)) {
                    const int nmore = (p <= 8 && n % 2) ? 2 : 0;
                    const uint64_t seed = mix(((uint64_t)c.dt << 40) ^ ((uint64_t)c.op << 32) ^ ((uint64_t)p << 24) ^ n);
                    auto add = [&](int off, unsigned nt) { out.push_back(TreeCase{c.dt, c.op, p, u, n, off, nmore, nt, seed}); };
                    if (n < 1000) { // the offsets are swept at the short lengths only
                        for (int off : offs) add(off, k++ & 1);
                        add(-1, k++ & 1);
                    } else if (n < 5000) {
                        add(offs[1 + k % (offs.size() - 1)], 0);
                        add(offs[1 + k % (offs.size() - 1)], 1);
                        add(-1, k++ & 1);
                    } else { // several workgroups: both kinds of store
                        add(offs[k % offs.size()], 0);
                        add(offs[k++ % offs.size()], 1);
                    }
                }
            }
    }
    return out;
}

// ---- tree_batch_kernel cases: ntree ragged trees, tree k at offsets[k % size], co-aligned ----
struct BatchCase {
    int dt, op, p;
    size_t n;
    int ntree;
    uint64_t seed;
    size_t tree_n(int k) const { return n + (size_t)k * 37; }
    size_t tree_off(int k) const
    {
        const std::vector<int> &o = offsets(esize(dt));
        return (size_t)o[(size_t)k % o.size()];
    }
    uint64_t tree_seed(int k) const { return mix(seed + (uint64_t)k); }
};
static const unsigned kBatchCaps[3] = {0, 64, 9};

inline std::vector<BatchCase> batch_cases()
{
    std::vector<BatchCase> out;
    for (const Combo &c : kCombos)
        for (int p : {2, 4, 8})
            for (size_t n : {(size_t)5, (size_t)4099, (size_t)(1u << 14) + 3})
                for (int nt : {1, 3, 8})
                    out.push_back(BatchCase{c.dt, c.op, p, n, nt,
                                            mix(0xba7cull ^ ((uint64_t)c.dt << 40) ^ ((uint64_t)c.op << 32) ^ ((uint64_t)p << 24) ^ (n << 4) ^ (uint64_t)nt)});
    return out;
}

// ---- segment lists -----------------------------------------------------------------------
struct SegPiece {
    size_t n;
    int kind; // 0 copy, 1 reduce
    bool with2;
    int ox, oy, oo, oo2; // byte offsets past a 16-byte boundary
    uint64_t seed;
};
struct SegList {
    int dt, op;
    unsigned cap;
    bool coalign;
    std::vector<SegPiece> pc;
};
static const unsigned kSegCaps[4] = {1u << 20, 1024, 128, 7};
constexpr int kSegLists = 210; // 15 rounds of the 14 combinations

inline SegList seg_list(int li)
{
    const Combo &c = kCombos[li % 14];
    const size_t es = esize(c.dt);
    const std::vector<int> &offs = offsets(es);
    uint64_t h = mix(0x5e95ull + (uint64_t)li);
    auto next = [&]() { return h = mix(h); };
    SegList L;
    L.dt = c.dt;
    L.op = c.op;
    // every fifth round (three lists per combination) is built to reach the interleaved prefix:
    // an uncapped grid and two long pieces at the head of the list, co-aligned at an offset
    // that leaves a vector body
    const bool ilv = (li / 14) % 5 == 4;
    L.cap = ilv ? kSegCaps[0] : kSegCaps[(li / 14 + li) % 4];
    L.coalign = next() % 4 != 0 || ilv;
    const int nseg = (ilv ? 2 : 1) + (int)(next() % 15);
    const int common = ilv ? offs[next() % (es == 16 ? 1 : 2)] : offs[next() % offs.size()];
    for (int s = 0; s < nseg; s++) {
        SegPiece P;
        // mostly short pieces; one in eight 256 KiB .. 2 MiB: several 128 KiB chunks of the interleaved prefix
        const bool big = next() % 8 == 0 || (ilv && s < 2);
        const size_t bytes = big ? (256u << 10) + next() % ((2u << 20) - (256u << 10)) : 1 + next() % 36000;
        P.n = std::max<size_t>(1, bytes / es);
        P.kind = next() % 3 == 0 ? 0 : 1;
        P.with2 = next() % 3 != 0;
        auto off = [&]() { return L.coalign ? common : offs[next() % offs.size()]; };
        P.ox = off();
        P.oy = off();
        P.oo = off();
        P.oo2 = off();
        P.seed = next();
        L.pc.push_back(P);
    }
    return L;
}

} // namespace kgen
