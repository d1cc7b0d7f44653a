// TEST-ONLY, host-only: the tables and inputs of gather_check (gather_kernel, gather_cvt_kernel and
// gather_mix_kernel, the movers of ftar_allreduce_multi, ftar_allreduce_multi_acc32 and
// ftar_allreduce_multi_mixed) and the cases of lds_check (reduce_lds_kernel), shared with ref_check, whose selftest replays every table on the CPU and
// asserts that the matrices reach what they are meant to reach and that the scatter inputs can
// tell a wrong narrowing from the right one (tests/test_kernel_ref.py).
//
// Nothing here uses the product's gather_first / gather_piece / cvt_piece: a table is a list of
// element counts and user offsets, its expectation plain concatenation.  Every input byte is a
// function of (seed, entry, element); no generator state.
//
// A table lives in one arena (256-byte aligned): a guard, the packed vector `pbase` bytes past a
// 256-byte boundary, a guard, then one 256-byte aligned slot per entry whose user buffer starts
// kGuard + uoff bytes into it.  A `pinned` table keeps its slots in a second arena of pinned host
// memory, laid out the same way from offset 0.  A mixed table (mix_tables()) gives every entry a
// type of its own: its packed side counts 4 bytes per element, its user side the type's own size.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "gen_types.h"

namespace kmov {
using kgen::Bytes;
using kgen::mix;
using namespace kref;

constexpr size_t kTile = 16384;      // ftar::kTileBytes (gather_check asserts it)
constexpr size_t kWave = 1024;       // kWavePiece of ftar_kernels.hip: below it a piece is one wave's
constexpr size_t kGuard = 64;        // around every user buffer
constexpr size_t kPackedGuard = 256; // around the packed vector
constexpr unsigned char kSentinel = 0xC3;
inline size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

enum Block { kMixed = 0, kPatterns = 1, kTies = 2, kNonFinite = 3 };

struct Table {
    std::string name;
    unsigned es = 4;    // packed bytes per element (the call's element size; 4 for a converting table)
    bool cvt = false;   // user elements are 2-byte floats
    size_t pbase = 0;   // the packed vector's first byte past a 256-byte boundary
    bool pinned = false;
    uint64_t seed = 0;
    int block = kMixed; // converting tables: what the leading elements hold
    size_t nlead = 0;   // ... and how many of them (the rest is the mixed fill)
    std::vector<size_t> cnt; // elements per entry
    std::vector<int> uoff;   // user buffer's byte offset past a 16-byte boundary
    std::vector<int> ty;     // a mixed table: kFloat16, kBFloat16 or kFloat32 per entry; empty: uniform
    bool mixed() const { return !ty.empty(); }
    bool two_byte(size_t e) const { return ty.empty() ? cvt : ty[e] != kFloat32; }
    size_t ues(size_t e) const { return ty.empty() ? (cvt ? 2 : es) : (ty[e] == kFloat32 ? 4 : 2); } // user bytes per element
    size_t elems() const
    {
        size_t n = 0;
        for (size_t c : cnt) n += c;
        return n;
    }
    size_t total() const { return elems() * es; }
};

struct Layout {
    size_t packed_at = 0, total = 0;
    std::vector<size_t> off, first; // packed byte offset and first element of every entry
    std::vector<size_t> sub;        // first element counted among those of the entry's kind (2-byte, or not)
    size_t n16 = 0, n32 = 0;        // elements of 2-byte entries / of the others
    std::vector<size_t> user_at;    // in the device arena, or in the pinned one
    size_t dev_bytes = 0, host_bytes = 0;
};

inline Layout layout(const Table &T)
{
    Layout L;
    L.packed_at = kPackedGuard + T.pbase;
    size_t o = 0, e0 = 0;
    for (size_t c : T.cnt) {
        L.off.push_back(o);
        L.first.push_back(e0);
        size_t &kind = T.two_byte(L.sub.size()) ? L.n16 : L.n32;
        L.sub.push_back(kind);
        kind += c;
        o += c * T.es;
        e0 += c;
    }
    L.total = o;
    size_t dev = round256(L.packed_at + L.total + kPackedGuard), host = 0;
    size_t &next = T.pinned ? host : dev;
    for (size_t i = 0; i < T.cnt.size(); i++) {
        L.user_at.push_back(next + kGuard + (size_t)T.uoff[i]);
        next += round256(T.cnt[i] * T.ues(i) + 16 + 2 * kGuard);
    }
    L.dev_bytes = dev;
    L.host_bytes = host;
    return L;
}

// ---- entry sizes ---------------------------------------------------------------------------
// V elements per 16-byte vector (plain) or per widest group (converting: 8).  One element; around
// one vector; around kWavePiece; around 4 * 64 and 4 * 256 vectors (the unrolled loops' exact
// ends); one tile and one element either side; then a filler up to the next tile edge, so that
// the entry in front of `3` ends exactly there; one entry over five tiles and a bit; a short one.
inline std::vector<size_t> main_counts(unsigned es, bool cvt)
{
    const size_t V = cvt ? 8 : 16 / es, T = kTile / es, W = kWave / es;
    std::vector<size_t> c = {1, V - 1, V, V + 1};
    if (cvt) {
        // K == 1 groups of one wave (4 * 64 - 1 = 255 is the most a piece below kWavePiece has),
        // then of the workgroup; the three of 1023 .. 1025 elements stay inside the first tile
        for (size_t n : {(size_t)193, W - 1, W, W + 1, (size_t)1023, (size_t)1024, (size_t)1025}) c.push_back(n);
        for (size_t n : {255 * V, 256 * V - 1, 256 * V, 256 * V + 1, 257 * V, T - 1, T, T + 1}) c.push_back(n);
    } else {
        for (size_t n : {(size_t)(1023 / es), W, W + 1, 255 * V, 256 * V, 257 * V, 258 * V, 1023 * V, T, 1025 * V, T - 1, T + 1})
            c.push_back(n);
    }
    std::vector<size_t> out;
    size_t sum = 0;
    for (size_t n : c)
        if (n) {
            out.push_back(n);
            sum += n;
        }
    out.push_back(T - sum % T); // ends exactly on a tile edge ...
    out.push_back(3);           // ... followed by another entry
    out.push_back(5 * T + 3);
    out.push_back(2);
    return out;
}

inline unsigned align_of(unsigned es) { return es < 8 ? es : (es == 8 ? 4 : 8); } // 8-byte pairs: 4; the 16-byte pair: 8

enum Mode { kSame, kCo, kOwn, kOddMix, kClass, kMixCo, kMixOff };

// user offsets of a table whose counts and pbase are set.  kSame: every entry at `arg`; kCo: every
// entry congruent to its packed address mod 16 (the vector path everywhere); kOwn: entry i at its
// own multiple of the alignment; kOddMix (2-byte elements, an odd packed address): every third
// entry congruent (odd, units of one byte with a vector body), the others even (bytes throughout);
// kClass (converting): element-index difference `arg` mod 8 between the packed and the user
// side -- 0, 4, 2 / 6, odd: class 8, 4, 2, 1.
inline void set_offsets(Table &T, Mode mode, int arg)
{
    const unsigned a = T.cvt ? 2 : align_of(T.es);
    size_t o = 0;
    T.uoff.clear();
    for (size_t i = 0; i < T.cnt.size(); i++) {
        const size_t pa = T.pbase + o;
        int u = 0;
        switch (mode) {
        case kSame: u = arg; break;
        case kCo: u = (int)(pa & 15); break;
        case kOwn: u = (int)((i * 7 % 16) / a * a); break;
        case kOddMix: u = i % 3 == 0 ? (int)(pa & 15) : (int)((i * 6) & 14); break;
        case kClass: u = (int)(2 * ((pa / 4 + 8 - (size_t)arg) & 7)); break;
        default: break; // (the mixed tables' modes: set_mix_offsets)
        }
        T.uoff.push_back(u);
        o += T.cnt[i] * T.es;
    }
}

inline std::vector<size_t> ones_counts(unsigned es)
{
    std::vector<size_t> c(320, 1); // 320 one-element entries inside the first tile, entry e on wave e & 3
    c.push_back(kTile / es);
    c.push_back(5);
    return c;
}
inline std::vector<size_t> max_counts()
{
    std::vector<size_t> c(1024); // ftar::kMaxGather entries
    for (size_t i = 0; i < 1024; i++) c[i] = 1 + i * 11 % 7 + (i % 97 == 0 ? 700 : 0);
    return c;
}

inline Table make(const std::string &name, unsigned es, bool cvt, const std::vector<size_t> &cnt, size_t pbase, Mode mode, int arg,
                  bool pinned = false)
{
    Table T;
    T.name = name;
    T.es = es;
    T.cvt = cvt;
    T.cnt = cnt;
    T.pbase = pbase;
    T.pinned = pinned;
    T.seed = mix(0x6a7be5ull ^ ((uint64_t)es << 32) ^ ((uint64_t)mode << 24) ^ ((uint64_t)(arg + 1) << 16) ^ (pbase << 4) ^ cnt.size());
    set_offsets(T, mode, arg);
    return T;
}

inline std::vector<Table> plain_tables()
{
    std::vector<Table> out;
    for (unsigned es : {2u, 4u, 8u, 16u, 1u}) { // (1: the 8-bit integers, appended behind the older tables)
        const unsigned a = align_of(es);
        const std::string s = "es" + std::to_string(es);
        const std::vector<size_t> main = main_counts(es, false), ones = ones_counts(es), many = max_counts();
        for (unsigned m = 0; m < 16; m += a) out.push_back(make(s + " main same " + std::to_string(m), es, false, main, 0, kSame, (int)m));
        // congruent everywhere, packed starts that leave a head: 6 (2-byte: 5 elements), 12 (4-byte: 1),
        // 4 (the 8-byte pairs: 12 bytes, an element split between the head and the vector body), 12
        // (the pairs again: 4 bytes), 8; and 0: whole aligned tiles of 1024 vectors
        for (size_t pb : es == 8 ? std::vector<size_t>{4, 12, 8} : es == 16 ? std::vector<size_t>{8, 0} : std::vector<size_t>{3 * a, 0})
            out.push_back(make(s + " main co " + std::to_string(pb), es, false, main, pb, kCo, 0, es == 4 && pb == 0));
        out.push_back(make(s + " main own", es, false, main, a, kOwn, 0));
        out.push_back(make(s + " ones co", es, false, ones, a, kCo, 0));
        out.push_back(make(s + " ones own pinned", es, false, ones, 0, kOwn, 0, true));
        out.push_back(make(s + " max own", es, false, many, 0, kOwn, 0));
        out.push_back(make(s + " max co", es, false, many, a, kCo, 0));
        if (es == 2) {
            out.push_back(make(s + " main odd packed", es, false, main, 1, kOddMix, 0));
            out.push_back(make(s + " ones odd packed", es, false, ones, 5, kOddMix, 0));
        }
    }
    return out;
}

inline std::vector<Table> cvt_tables()
{
    std::vector<Table> out;
    const std::vector<size_t> main = main_counts(4, true), ones = ones_counts(4), many = max_counts();
    for (int m = 0; m < 16; m += 2)
        out.push_back(make("cvt main same " + std::to_string(m), 4, true, main, (size_t)(4 * (m * 3 / 2 % 8)), kSame, m));
    const int cls[6] = {0, 4, 2, 6, 1, 3};
    for (int k = 0; k < 6; k++)
        out.push_back(make("cvt main class " + std::to_string(cls[k]), 4, true, main, (size_t)(4 * (k + 1)), kClass, cls[k], k == 1));
    out.push_back(make("cvt main own", 4, true, main, 20, kOwn, 0));
    out.push_back(make("cvt ones own pinned", 4, true, ones, 4, kOwn, 0, true));
    out.push_back(make("cvt ones class 0", 4, true, ones, 12, kClass, 0));
    out.push_back(make("cvt max own", 4, true, many, 8, kOwn, 0));
    out.push_back(make("cvt max class 4", 4, true, many, 28, kClass, 4));
    {
        // every 16-bit pattern, element j the pattern j, over entries of every class; then mixed
        std::vector<size_t> c = {1, 4095, 4099, 8189, 16384, 32768 - 13, 13, 5000};
        Table T = make("cvt patterns", 4, true, c, 4, kOwn, 0);
        T.block = kPatterns;
        T.nlead = 65536;
        out.push_back(T);
    }
    {
        // every pattern's tie with its neighbour away from zero and that tie -1 / +1 ulp of float32:
        // element 3 v + d; then mixed
        std::vector<size_t> c = {3 * 4096 + 1, 3 * 20000, 3 * 41436 - 1, 7000};
        Table T = make("cvt ties", 4, true, c, 16, kOwn, 0);
        T.block = kTies;
        T.nlead = 3 * 65536;
        out.push_back(T);
    }
    {
        // block F: infinities and NaNs only (exempt from the NaN cap by this name; below 257 elements)
        std::vector<size_t> c = {61, 70, 1, 69};
        Table T = make("cvt nonfinite", 4, true, c, 8, kOwn, 0);
        T.block = kNonFinite;
        T.nlead = T.elems();
        out.push_back(T);
    }
    return out;
}

// ---- mixed tables (gather_mix_kernel) ---------------------------------------------------------
// Packed offsets and sizes count 4 bytes per element for every entry (es = 4), the user side 2 or
// 4.  kSame: every entry at `arg`, a float32 entry at `arg` rounded down to a multiple of 4; kOwn as
// above with the entry's own alignment; kMixCo: every float32 entry congruent to its packed address
// mod 16 (the vector path) and every 2-byte entry of class 8; kMixOff: no float32 entry congruent
// (words throughout), the 2-byte ones of class 4, 2 and 1 in turn.
inline const char *type_name(int dt) { return dt == kFloat16 ? "float16" : dt == kBFloat16 ? "bfloat16" : "float32"; }
inline int type_index(int dt) { return dt == kFloat16 ? 0 : dt == kBFloat16 ? 1 : 2; }
static const int kMixTypes[3] = {kFloat16, kBFloat16, kFloat32};

inline void set_mix_offsets(Table &T, Mode mode, int arg)
{
    static const size_t diff[5] = {4, 2, 1, 6, 3}; // element-index differences: class 4, 2, 1, 2, 1
    size_t o = 0;
    T.uoff.clear();
    for (size_t i = 0; i < T.cnt.size(); i++) {
        const size_t pa = T.pbase + o, turn = i + i / 3;
        const bool f32 = T.ty[i] == kFloat32;
        const int a = f32 ? 4 : 2;
        int u = 0;
        switch (mode) {
        case kSame: u = arg / a * a; break;
        case kOwn: u = (int)(i * 7 % 16) / a * a; break;
        case kMixCo: u = f32 ? (int)(pa & 15) : (int)(2 * ((pa / 4) & 7)); break;
        default: u = f32 ? (int)((pa + 4 + 4 * (turn % 3)) & 15) : (int)(2 * ((pa / 4 + 8 - diff[turn % 5]) & 7)); break;
        }
        T.uoff.push_back(u);
        o += T.cnt[i] * 4;
    }
}

inline std::vector<int> type_cycle(size_t n, const std::vector<int> &period, size_t start = 0)
{
    std::vector<int> ty(n);
    for (size_t i = 0; i < n; i++) ty[i] = period[(i + start) % period.size()];
    return ty;
}

inline Table make_mix(const std::string &name, const std::vector<size_t> &cnt, const std::vector<int> &ty, size_t pbase, Mode mode,
                      int arg, bool pinned = false)
{
    Table T;
    T.name = name;
    T.es = 4;
    T.cnt = cnt;
    T.ty = ty;
    T.pbase = pbase;
    T.pinned = pinned;
    uint64_t h = 0x3a1d7ull;
    for (char c : name) h = mix(h ^ (unsigned char)c);
    T.seed = h;
    set_mix_offsets(T, mode, arg);
    return T;
}

// the 2-byte entries of a value table with float32 entries of 1, 5 and 4099 elements between them
inline void interleave_f32(const std::vector<size_t> &c16, int dt16, std::vector<size_t> *cnt, std::vector<int> *ty)
{
    static const size_t between[3] = {1, 5, 4099};
    for (size_t i = 0; i < c16.size(); i++) {
        if (i) {
            cnt->push_back(between[(i - 1) % 3]);
            ty->push_back(kFloat32);
        }
        cnt->push_back(c16[i]);
        ty->push_back(dt16);
    }
}

inline std::vector<Table> mix_tables()
{
    std::vector<Table> out;
    const std::vector<int> three(kMixTypes, kMixTypes + 3);
    const std::vector<size_t> main = main_counts(4, true), ones = ones_counts(4), many = max_counts();
    const size_t starts[5] = {0, 4, 8, 12, 20}, T = kTile / 4;
    // main: every size with every type (the cycle started at each), every user offset, the packed
    // starts that give a congruent float32 entry heads of 0, 3, 2 and 1 words.  Entry 17 (one tile)
    // is float32 in cycle 0, entry 21 (five tiles + 3, starting 12 bytes behind a tile edge) in
    // cycle 2: whole tiles of 1024 vectors at packed start 0, of 1023 with head and tail at 4.
    for (size_t s = 0; s < 3; s++) {
        const std::string c = "mix main cycle " + std::to_string(s);
        const std::vector<int> ty = type_cycle(main.size(), three, s);
        for (int m = 0; m < 16; m += 2) out.push_back(make_mix(c + " same " + std::to_string(m), main, ty, starts[(m / 2 + s) % 5], kSame, m));
        out.push_back(make_mix(c + " own", main, ty, starts[(s + 3) % 5], kOwn, 0, s == 1)); // (cycle 1: pinned)
        for (size_t pb : starts) out.push_back(make_mix(c + " co " + std::to_string(pb), main, ty, pb, kMixCo, 0));
        out.push_back(make_mix(c + " off", main, ty, starts[s + 1], kMixOff, 0));
    }
    // ones: with a period of 3 every (wave, type) pair occurs; with {f16, f32, bf16, f32} every wave
    // sees one type only -- an index by wave where the entry's is meant shows in one of the two
    out.push_back(make_mix("mix ones period 3 co", ones, type_cycle(ones.size(), three), 12, kMixCo, 0));
    out.push_back(make_mix("mix ones period 3 own pinned", ones, type_cycle(ones.size(), three, 1), 0, kOwn, 0, true));
    out.push_back(make_mix("mix ones period 4 own", ones, type_cycle(ones.size(), {kFloat16, kFloat32, kBFloat16, kFloat32}), 4, kOwn, 0));
    out.push_back(make_mix("mix ones period 4 co", ones, type_cycle(ones.size(), {kFloat16, kFloat32, kBFloat16, kFloat32}), 8, kMixCo, 0));
    // the type array begins 24 n bytes behind the table: n = 1024, 1023 and 7
    out.push_back(make_mix("mix max own", many, type_cycle(many.size(), three), 8, kOwn, 0));
    out.push_back(make_mix("mix max co", many, type_cycle(many.size(), three, 2), 20, kMixCo, 0));
    out.push_back(make_mix("mix 1023 entries", std::vector<size_t>(many.begin(), many.begin() + 1023), type_cycle(1023, three, 1), 4, kOwn, 0));
    out.push_back(make_mix("mix 7 entries", std::vector<size_t>(many.begin(), many.begin() + 7), type_cycle(7, three, 2), 12, kMixCo, 0));
    // a tile edge exactly between two types, and one 3 elements before the first type's end; two
    // neighbours of one type behind them
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            if (a == b) continue;
            const int A = kMixTypes[a], B = kMixTypes[b];
            const std::string ab = std::string(type_name(A)) + " | " + type_name(B);
            out.push_back(make_mix("mix edge between " + ab, {7, T - 7, 600, 9, 5}, {B, A, B, A, A}, starts[(size_t)(a + b) % 5], a < b ? kMixCo : kOwn, 0));
            out.push_back(make_mix("mix edge inside " + ab, {7, T - 4, 600, 9, 5}, {B, A, B, A, A}, starts[(size_t)(a + 2 * b) % 5], a < b ? kOwn : kMixCo, 0));
        }
    // the kWavePiece threshold in packed bytes: 1020, 1024, 1028 for every type, next to each other
    // in one tile; the three one-wave pieces (entries 0, 3, 6) on waves 0, 3 and 2
    {
        std::vector<size_t> c;
        std::vector<int> ty;
        for (int t : kMixTypes)
            for (size_t n : {(size_t)255, (size_t)256, (size_t)257}) {
                c.push_back(n);
                ty.push_back(t);
            }
        out.push_back(make_mix("mix thresholds co", c, ty, 0, kMixCo, 0));
        out.push_back(make_mix("mix thresholds off", c, ty, 8, kMixOff, 0));
    }
    // the converting tables' value blocks in the 2-byte entries (every pattern; every tie; infinities
    // and NaNs), once per 2-byte type, with float32 entries between them
    for (int dt : {(int)kFloat16, (int)kBFloat16}) {
        const std::string t = type_name(dt);
        struct { const char *name; std::vector<size_t> c16; size_t pbase; int block; size_t nlead; } v[3] = {
            {"mix patterns ", {1, 4095, 4099, 8189, 16384, 32768 - 13, 13, 5000}, 4, kPatterns, 65536},
            {"mix ties ", {3 * 4096 + 1, 3 * 20000, 3 * 41436 - 1, 7000}, 16, kTies, 3 * 65536},
            {"mix nonfinite ", {61, 70, 1, 69}, 8, kNonFinite, 201}};
        for (const auto &b : v) {
            std::vector<size_t> c;
            std::vector<int> ty;
            interleave_f32(b.c16, dt, &c, &ty);
            Table V = make_mix(b.name + t, c, ty, b.pbase, kOwn, 0);
            V.block = b.block;
            V.nlead = b.nlead;
            out.push_back(V);
        }
    }
    return out;
}

inline std::vector<unsigned> grids(unsigned ntiles)
{
    std::vector<unsigned> g = {ntiles};
    for (unsigned c : {7u, 1u}) {
        const unsigned v = c < ntiles ? c : ntiles;
        if (v != g.back()) g.push_back(v);
    }
    return g;
}

// ---- plain mover: bytes ----------------------------------------------------------------------
// byte b of entry e's user buffer (gather) / packed byte b (scatter: entry = ~0)
inline unsigned char plain_byte(uint64_t seed, uint64_t entry, size_t b)
{
    return (unsigned char)(mix(seed ^ mix(entry * 0x100000001ull + b / 8)) >> (8 * (b % 8)));
}

// ---- converting mover ------------------------------------------------------------------------
static const float kScales[7] = {1.0f, 0.5f, 1.0f / 3.0f, -1.0f, 0x1p-12f, 0.0f, 3.0000002f};
inline bool exact_scale(float s) { return s == 1.0f || s == -1.0f || s == 0.5f || s == 0x1p-12f; }

inline float f32_of(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// magnitude k of the format read as if the exponent field had no special value: k = the infinity's
// pattern gives the power of two above the largest finite value
inline double mag16(int dt, unsigned k)
{
    const int mb = mant_bits(dt), bias = (1 << (exp_bits(dt) - 1)) - 1;
    const int e = (int)(k >> mb), m = (int)(k & ((1u << mb) - 1));
    if (e == 0) return (double)m * pow2(1 - bias - mb);
    return (double)((1 << mb) + m) * pow2(e - bias - mb);
}
inline unsigned inf16(int dt) { return (unsigned)(((1 << exp_bits(dt)) - 1) << mant_bits(dt)); }

// the float32 halfway between magnitude k (finite) and k + 1: exact (at most 12 significant bits,
// and no smaller than 2^-134 for bfloat16, 2^-25 for float16)
inline float tie16(int dt, unsigned k) { return (float)((mag16(dt, k) + mag16(dt, k + 1)) * 0.5); }

// the gather's user pattern at element g of a table
inline uint16_t cvt_user(const Table &T, size_t g)
{
    if (T.block == kPatterns && g < T.nlead) return (uint16_t)g;
    return (uint16_t)(g * 40503u + (unsigned)(T.seed >> 8)); // an odd stride: every pattern once in 65536 elements
}

// a float32 a whose product scale * a is the target t, or rounds to it in float32 where such an a
// is found within two ulps of t / scale (then, the scale not being a power of two, the exact
// product is mostly NOT t: one rounding into the 16-bit type and two roundings part ways)
inline float toward(float t, float scale)
{
    if (scale == 0.0f || std::isnan(t) || std::isinf(t)) return t;
    const float a0 = (float)((double)t / (double)scale);
    if (exact_scale(scale) || std::isinf(a0) || a0 == 0.0f) return a0;
    for (int d : {0, 1, -1, 2, -2}) {
        const float a = f32_of(bits_of(a0) + (uint32_t)d);
        if ((float)((double)scale * (double)a) == t) return a;
    }
    return a0;
}

// packed float32 element g of a scatter at this scale
inline float cvt_packed(const Table &T, int dt, float scale, size_t g)
{
    const uint64_t h = mix(T.seed ^ mix(((uint64_t)dt << 56) ^ g)), h2 = mix(h);
    const unsigned inf = inf16(dt), sgn = (unsigned)(h >> 8) & 1;
    auto widened = [&](uint16_t p) { return (float)decode16(p, dt); };
    auto sign = [&](float v) { return sgn ? -v : v; };
    if (g < T.nlead) {
        if (T.block == kPatterns) return widened((uint16_t)g);
        if (T.block == kTies) {
            const unsigned v = (unsigned)(g / 3), k = v & 0x7fff;
            if (k >= inf) return widened((uint16_t)v);
            const float t = f32_of(bits_of(tie16(dt, k)) + (uint32_t)(g % 3) - 1u);
            return toward((v & 0x8000) ? -t : t, scale);
        }
        switch (g % 10) { // block F
        case 0: return INFINITY;
        case 1: return -INFINITY;
        case 2: return f32_of(0x7f800001u); // the upper 16 bits alone read as an infinity
        case 3: return f32_of(0xff800001u);
        case 4: return f32_of(0x7fc00000u | (uint32_t)(h & 0x3fffff));
        case 5: return f32_of(0xff800000u | (uint32_t)(h & 0x7fffff) | 1u);
        case 6: return f32_of(0x7f80ffffu);
        case 7: return sign(3.4028234663852886e38f);
        case 8: return f32_of(0x7f810000u);
        default: return sign(INFINITY);
        }
    }
    const unsigned c = (unsigned)(h % 32);
    if (c < 6) { // a widened 16-bit pattern as it is; a NaN or an infinity one time in four of the few
        uint16_t p = (uint16_t)(h >> 16);
        if ((p & inf) == inf && (h >> 40) % 4) p &= (uint16_t)~(1u << mant_bits(dt));
        return widened(p);
    }
    if (c < 14) { // A: a tie of a finite pattern, -1 / 0 / +1 ulp of float32
        const unsigned k = (unsigned)(h >> 16) % inf;
        return toward(sign(f32_of(bits_of(tie16(dt, k)) + (uint32_t)((h >> 40) % 3) - 1u)), scale);
    }
    if (c < 17) { // B: ties in the subnormal range, down to half the smallest subnormal
        const unsigned k = (unsigned)(h >> 16) % (c == 14 ? 2u : (1u << mant_bits(dt)));
        return toward(sign(f32_of(bits_of(tie16(dt, k)) + (uint32_t)((h >> 40) % 3) - 1u)), scale);
    }
    if (c == 17) { // C: the overflow edge
        const float tie = tie16(dt, inf - 1);
        const float v[5] = {(float)mag16(dt, inf - 1), tie, f32_of(bits_of(tie) - 1), f32_of(bits_of(tie) + 1), 3.4028234663852886e38f};
        const unsigned w = (unsigned)(h >> 16) % 5;
        return w == 4 ? sign(v[4]) : toward(sign(v[w]), scale);
    }
    if (c == 18 || c == 19) { // D: -0, and values whose product is negative and underflows to -0
        const bool neg_scale = std::signbit(scale);
        switch ((h >> 16) % 4) {
        case 0: return neg_scale ? 0.0f : -0.0f;
        case 1: return neg_scale ? f32_of(1) : f32_of(0x80000001u);            // float32's smallest subnormal
        case 2: return f32_of((neg_scale ? 0u : 0x80000000u) | (1u + (uint32_t)(h2 % 0x7fff))); // below every bfloat16 tie
        default: return (neg_scale ? 1.0f : -1.0f) * (dt == kFloat16 ? 0x1p-26f : 0x1p-140f);  // below half the smallest subnormal
        }
    }
    if (c == 20 || c == 21) { // E: a product in float32's subnormal range (|a| ~ 2^-120 at scale 2^-12)
        const float t = f32_of((uint32_t)(0x00010000u + (h2 % 0x007f0000u)));
        return scale == 0x1p-12f ? sign(t * 0x1p12f) : toward(sign(t), scale);
    }
    // a random value of 2^-16 .. 2^15 with a full mantissa
    const float t = f32_of((uint32_t)((127 - 16 + (h2 >> 32) % 31) << 23) | (uint32_t)(h2 & 0x7fffff));
    return toward(sign(t), scale);
}

// The contract (include/ftar.h, step 3): ONE float32 multiplication, ONE conversion.  The double
// product of two float32 values is exact, the cast to float the multiplication's rounding.
enum Narrow { kContract = 0, kFused = 4, kPlusZero = 5, kUpperHalf = 6 }; // 1 .. 3: kref::Round's mutants
inline uint16_t narrow_ref(float a, float scale, int dt, int how = kContract)
{
    const double exact = (double)scale * (double)a;
    const float prod = (float)exact;
    if (how == kFused) return encode16(exact, dt);
    if (how == kPlusZero && prod == 0.0f) return 0;
    // (the multiplication quiets a signalling NaN: the mutant is one that looks at a's upper half)
    if (how == kUpperHalf && scale != 0.0f && (bits_of(a) & 0x7fff0000u) == 0x7f800000u)
        return (uint16_t)(((bits_of(a) ^ bits_of(scale)) >> 31 << 15) | inf16(dt));
    return encode16((double)prod, dt, how >= 1 && how <= 3 ? (Round)how : kNearestEven);
}

// ---- mixed mover: the float32 entries ----------------------------------------------------------
// gather: word i of entry e's user buffer -- arbitrary bits, one in eight a signalling NaN and one
// in eight a quiet NaN with a payload.  A gather is a copy: the expectation is the same bits.
inline uint32_t f32_user(const Table &T, size_t e, size_t i)
{
    uint32_t w = 0;
    for (size_t b = 0; b < 4; b++) w |= (uint32_t)plain_byte(T.seed, e, 4 * i + b) << (8 * b);
    const uint64_t h = mix(T.seed ^ mix(0xf32ull + e * 0x9e3779b97f4a7c15ull + i));
    if (h % 8 == 0) return (w & 0x803fffffu) | 0x7f800000u | 1u; // signalling: the quiet bit clear
    if (h % 8 == 1) return w | 0x7fc00000u;
    return w;
}
inline bool signalling(uint32_t w) { return (w & 0x7fc00000u) == 0x7f800000u && (w & 0x003fffffu); }

// scatter: packed float32 element g (counted among the float32 elements) at this scale
inline float f32_packed(const Table &T, float scale, size_t g)
{
    const uint64_t h = mix(T.seed ^ mix(((uint64_t)kFloat32 << 56) ^ g)), h2 = mix(h);
    const unsigned c = (unsigned)(h % 64), sgn = (unsigned)(h >> 8) & 1;
    const bool neg_scale = std::signbit(scale);
    auto sign = [&](float v) { return sgn ? -v : v; };
    if (c < 2) return sign(0.0f);
    if (c < 6) { // a product in float32's subnormal range
        const float t = f32_of((uint32_t)(0x00010000u + (h2 % 0x007f0000u)));
        return scale == 0x1p-12f ? sign(t * 0x1p12f) : toward(sign(t), scale);
    }
    if (c < 9) // -0, and values whose product is negative and underflows to -0 at the small scales
        switch ((h >> 16) % 3) {
        case 0: return neg_scale ? 0.0f : -0.0f;
        case 1: return neg_scale ? f32_of(1) : f32_of(0x80000001u);
        default: return f32_of((neg_scale ? 0u : 0x80000000u) | (1u + (uint32_t)(h2 % 0x3f)));
        }
    if (c < 11) return sign(f32_of(0x7eaaaaaau + 256u + (uint32_t)(h2 % 1000))); // a third of the largest value and a bit: overflows at 3.0000002
    if (c == 11) return sign(INFINITY);                                             // a NaN at scale 0
    if (c == 12) return f32_of(0x7fc00000u | (uint32_t)(h2 & 0x803fffffu));
    if (c == 13) return f32_of(0x7f800000u | (uint32_t)(h2 & 0x803fffffu) | 1u);  // signalling
    if (c == 14) return sign(3.4028234663852886e38f);
    return sign(f32_of((uint32_t)((127 - 16 + (h2 >> 32) % 31) << 23) | (uint32_t)(h2 & 0x7fffff))); // 2^-16 .. 2^15, a full mantissa
}

// The contract of a float32 entry (include/ftar.h): ONE float32 multiplication.  Mutants: the
// Narrow ones that apply (kPlusZero) and two of its own.
enum ScaleMutant { kFlushProduct = 7, kNotScaled = 8 };
inline uint32_t scale_ref(float a, float scale, int how = kContract)
{
    if (how == kNotScaled) return bits_of(a);
    const float prod = (float)((double)scale * (double)a);
    if (how == kPlusZero && prod == 0.0f) return 0;
    if (how == kFlushProduct && prod != 0.0f && std::fabs(prod) < 0x1p-126f) return bits_of(prod) & 0x80000000u;
    return bits_of(prod);
}

// ---- reduce_lds_kernel cases -----------------------------------------------------------------
struct LdsCombo { int dt, op; };
inline std::vector<LdsCombo> lds_combos()
{
    std::vector<LdsCombo> out;
    for (int dt : {kInt32, kInt64})
        for (int op = 0; op < 10; op++) out.push_back({dt, op});
    for (int dt : {kFloat32, kFloat64, kFloat16, kBFloat16})
        for (int op = 0; op < 4; op++) out.push_back({dt, op});
    for (int dt : {kFloatInt, k2Int, kDoubleInt})
        for (int op : {kMaxloc, kMinloc}) out.push_back({dt, op});
    return out;
}
static const size_t kLdsVecs[10] = {1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 4 * 1024 + 65};
constexpr size_t kLdsTileVecs = 1024;
inline std::vector<unsigned> lds_grids(size_t nv)
{
    const unsigned nt = (unsigned)((nv + kLdsTileVecs - 1) / kLdsTileVecs);
    std::vector<unsigned> g = {nt};
    for (unsigned c : {3u, 1u}) {
        const unsigned v = c < nt ? c : nt;
        if (v != g.back()) g.push_back(v);
    }
    return g;
}
inline uint64_t lds_seed(int dt, int op, size_t nv) { return mix(0x1d5ull ^ ((uint64_t)dt << 40) ^ ((uint64_t)op << 32) ^ nv); }

// the four types of the oracle: operand j (0: inout, 1: in), element i.  Integers: 0, 1, -1, the
// extremes and random bits (zeros matter to the logical ops); floats: random values, +-0, and for
// MAX / MIN NaNs of both signs and infinities, for SUM / PROD a sparse inf (inf - inf, inf * 0).
inline void fill_old(unsigned char *buf, int dt, int op, size_t n, int j, uint64_t seed)
{
    for (size_t i = 0; i < n; i++) {
        const uint64_t h = mix(seed ^ mix(i * 2 + (uint64_t)j)), h2 = mix(h);
        const unsigned c = (unsigned)(h % 16);
        if (dt == kInt32 || dt == kInt64) {
            int64_t v = (int64_t)h2;
            if (c < 3) v = (int64_t)c - 1;
            else if (c == 3) v = dt == kInt32 ? INT32_MAX : INT64_MAX;
            else if (c == 4) v = dt == kInt32 ? INT32_MIN : INT64_MIN;
            else if (c == 5) v = (int64_t)(h2 % 7) - 3;
            if (dt == kInt32) {
                const int32_t w = (int32_t)v;
                memcpy(buf + 4 * i, &w, 4);
            } else {
                memcpy(buf + 8 * i, &v, 8);
            }
            continue;
        }
        const bool sel = op == kMax || op == kMin;
        double v = std::ldexp((double)(int64_t)(h2 % 2000001) - 1000000.0, -(int)((h2 >> 32) % 20));
        if (op == kProd) v = 1.0 + std::ldexp((double)(int64_t)(h2 % 4097) - 2048.0, -12);
        uint64_t nanbits = 0x7ff8000000000000ull | ((h2 & 1) << 63) | ((h2 >> 20) & 0xffff);
        if (c == 0) v = 0.0;
        else if (c == 1) v = -0.0;
        else if (sel && (c == 2 || c == 3)) memcpy(&v, &nanbits, 8);
        else if (sel && c == 4) v = INFINITY;
        else if (sel && c == 5) v = -INFINITY;
        else if (sel && c == 6) v = (double)(int)(h2 % 3); // a few values on both sides: ties
        else if (!sel && i % 211 == 50) v = ((h2 >> 8) & 1) ? INFINITY : -INFINITY;
        if (dt == kFloat32) {
            const float f = (float)v;
            memcpy(buf + 4 * i, &f, 4);
        } else {
            memcpy(buf + 8 * i, &v, 8);
        }
    }
}

inline bool lds_old(int dt) { return dt == kInt32 || dt == kFloat32 || dt == kInt64 || dt == kFloat64; }
inline void lds_fill(unsigned char *buf, int dt, int op, size_t n, int j, uint64_t seed)
{
    if (lds_old(dt)) fill_old(buf, dt, op, n, j, seed);
    else kgen::fill(buf, dt, op, n, j, 2, seed);
}
// the result depends on which operand is `inout`
inline bool lds_order_sensitive(const LdsCombo &c)
{
    if (lds_old(c.dt)) return (c.dt == kFloat32 || c.dt == kFloat64) && (c.op == kMax || c.op == kMin);
    return kgen::order_sensitive(kgen::Combo{c.dt, c.op});
}
// elements that differ, by NaN-ness where a float SUM / PROD expectation is a NaN
inline size_t lds_diff(const unsigned char *got, const unsigned char *want, int dt, int op, size_t n, size_t *first = nullptr)
{
    if (!lds_old(dt)) return kgen::count_diff(got, want, dt, op, n, first);
    const size_t es = esize(dt);
    const bool nanness = (dt == kFloat32 || dt == kFloat64) && (op == kSum || op == kProd);
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        bool same = !memcmp(got + i * es, want + i * es, es);
        if (!same && nanness) {
            if (dt == kFloat32) {
                float g, w;
                memcpy(&g, got + 4 * i, 4);
                memcpy(&w, want + 4 * i, 4);
                same = std::isnan(g) && std::isnan(w);
            } else {
                double g, w;
                memcpy(&g, got + 8 * i, 8);
                memcpy(&w, want + 8 * i, 8);
                same = std::isnan(g) && std::isnan(w);
            }
        }
        if (!same && !bad++ && first) *first = i;
    }
    return bad;
}

} // namespace kmov
