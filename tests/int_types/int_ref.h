// TEST-ONLY: the 8-, 16-bit and unsigned integer types in plain C++ -- the reference `apply`, the
// inputs of every case of int_check (the GPU checker) and the wrong kernels those inputs must
// expose.  Header only, no HIP: shared by ref_check (host) and int_check (GPU).
//
// Reference.  include/ftar.h's rules written on uint64_t carriers, nothing shared with the
// kernels: SUM / PROD in uint64_t, masked to the width (modulo 2^w, signed and unsigned alike);
// MAX / MIN after sign- or zero-extension, `(x > y) ? x : y` with x = inout, y = in; the logical
// ops 0 / 1; the bitwise ops on the bits.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace iref {

enum { kInt8 = 48, kUInt8 = 49, kInt16 = 50, kUInt16 = 51, kUInt32 = 52, kUInt64 = 53 };
enum { kSum = 0, kProd = 1, kMax = 2, kMin = 3, kLand = 4, kBand = 5, kLor = 6, kBor = 7, kLxor = 8, kBxor = 9 };
constexpr int kTypes[] = {kInt8, kUInt8, kInt16, kUInt16, kUInt32, kUInt64};
constexpr int kNumOps = 10;

inline size_t esize(int dt)
{
    switch (dt) {
    case kInt8: case kUInt8: return 1;
    case kInt16: case kUInt16: return 2;
    case kUInt32: return 4;
    case kUInt64: return 8;
    default: return 0;
    }
}
inline bool is_signed(int dt) { return dt == kInt8 || dt == kInt16; }
inline uint64_t mask_of(int dt) { return esize(dt) == 8 ? ~0ull : (1ull << (8 * esize(dt))) - 1; }
inline int64_t widen(int dt, uint64_t v) // the value as the type reads it (uint64: see below)
{
    const unsigned w = 8 * (unsigned)esize(dt);
    if (is_signed(dt) && ((v >> (w - 1)) & 1)) return (int64_t)(v | ~mask_of(dt));
    return (int64_t)v;
}

// x = inout, y = in, both already masked to the width
inline uint64_t apply(int dt, int op, uint64_t x, uint64_t y)
{
    const uint64_t m = mask_of(dt);
    switch (op) {
    case kSum: return (x + y) & m;
    case kProd: return (x * y) & m;
    case kMax:
    case kMin: {
        bool gt, lt;
        if (dt == kUInt64) gt = x > y, lt = x < y;
        else gt = widen(dt, x) > widen(dt, y), lt = widen(dt, x) < widen(dt, y);
        return op == kMax ? (gt ? x : y) : (lt ? x : y);
    }
    case kLand: return (x != 0) && (y != 0);
    case kBand: return x & y;
    case kLor: return (x != 0) || (y != 0);
    case kBor: return x | y;
    case kLxor: return (x != 0) != (y != 0);
    default: return x ^ y;
    }
}

inline uint64_t get(const unsigned char *p, size_t es)
{
    uint64_t v = 0;
    memcpy(&v, p, es); // little-endian
    return v;
}
inline void put(unsigned char *p, size_t es, uint64_t v) { memcpy(p, &v, es); }

// inout[i] = inout[i] op in[i]
inline void reduce_local(int dt, int op, const unsigned char *in, unsigned char *inout, size_t n)
{
    const size_t es = esize(dt);
    for (size_t i = 0; i < n; i++) put(inout + i * es, es, apply(dt, op, get(inout + i * es, es), get(in + i * es, es)));
}

// The product's tree: ((s0 op s1) op (s2 op s3)) op ... over p sources (ftar_kernels.h, TreeArgs)
inline void tree(int dt, int op, int p, const unsigned char *const *src, unsigned char *out, size_t n)
{
    const size_t es = esize(dt);
    for (size_t i = 0; i < n; i++) {
        uint64_t v[16];
        for (int j = 0; j < p; j++) v[j] = get(src[j] + i * es, es);
        for (int w = 1; w < p; w <<= 1)
            for (int j = 0; j < p; j += 2 * w) v[j] = apply(dt, op, v[j], v[j + w]);
        put(out + i * es, es, v[0]);
    }
}

// ---- wrong kernels ------------------------------------------------------------------------
// Each is the reference with ONE mistake a packed or SWAR implementation can make; `applies`
// says for which (type, op) it differs from the reference at all.  They work on whole buffers:
// two of them leak between neighbouring elements of one 32-bit register (elements grouped by
// index from the start of the buffer).
enum { kSwappedSign = 0, kSaturating = 1, kCarryLeak = 2, kHighHalfKept = 3, kLogicalNotOne = 4, kNumMutants = 5 };
inline const char *mutant_name(int m)
{
    static const char *const names[] = {"signedness of the compare swapped", "saturating instead of wrapping",
                                        "a SWAR carry leaking into the neighbouring element",
                                        "a product's upper half not discarded", "a logical op returning a value other than 0 / 1"};
    return names[m];
}
inline bool applies(int m, int dt, int op)
{
    switch (m) {
    case kSwappedSign: return op == kMax || op == kMin;
    case kSaturating: return op == kSum || op == kProd;
    case kCarryLeak: return op == kSum && esize(dt) <= 2;
    case kHighHalfKept: return op == kProd && esize(dt) <= 2;
    default: return op == kLand || op == kLor || op == kLxor;
    }
}
inline void mutant_reduce(int m, int dt, int op, const unsigned char *in, unsigned char *inout, size_t n)
{
    const size_t es = esize(dt);
    const uint64_t mk = mask_of(dt);
    const unsigned w = 8 * (unsigned)es;
    const size_t per = es <= 2 ? 4 / es : 1; // elements of one 32-bit register
    uint64_t carry = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t x = get(inout + i * es, es), y = get(in + i * es, es);
        uint64_t r = apply(dt, op, x, y);
        if (i % per == 0) carry = 0;
        switch (m) {
        case kSwappedSign: {
            const uint64_t flip = 1ull << (w - 1); // order of the other signedness
            const bool gt = (x ^ flip) > (y ^ flip), lt = (x ^ flip) < (y ^ flip);
            const bool s = is_signed(dt); // signed: compare as unsigned; unsigned: as signed
            const bool g2 = s ? x > y : gt, l2 = s ? x < y : lt;
            r = op == kMax ? (g2 ? x : y) : (l2 ? x : y);
            break;
        }
        case kSaturating:
            if (is_signed(dt)) {
                const __int128 a = widen(dt, x), b = widen(dt, y), v = op == kSum ? a + b : a * b;
                const __int128 hi = (__int128)(mk >> 1), lo = -hi - 1;
                r = (uint64_t)(int64_t)(v > hi ? hi : v < lo ? lo : v) & mk;
            } else {
                const unsigned __int128 v = op == kSum ? (unsigned __int128)x + y : (unsigned __int128)x * y;
                r = v > mk ? mk : (uint64_t)v;
            }
            break;
        case kCarryLeak: {
            const uint64_t s = x + y + carry;
            r = s & mk;
            carry = s >> w;
            break;
        }
        case kHighHalfKept: {
            const uint64_t pr = x * y; // es <= 2: exact in 64 bits
            r = (pr + carry) & mk;
            carry = pr >> w;
            break;
        }
        default:
            if (r) r = (x | y) & mk; // "true" as whatever bits were at hand
            break;
        }
        put(inout + i * es, es, r);
    }
}

// ---- inputs -------------------------------------------------------------------------------
inline uint64_t mix(uint64_t z) // splitmix64
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// Operand `which` (0 = x / inout / source 0, 1 = y / in / source 1, 2.. further sources) of n
// elements.  The first elements are pairs chosen per op so that a case of five elements already
// separates the reference from every wrong kernel above: the extremes of both signednesses against
// each other (MAX / MIN), sums and products that pass 2^(w-1) and 2^w with a neighbour to leak
// into, non-zero operands without a common bit (logical).  Behind them: half the elements from the
// values around 0, 2^(w-1) and 2^w - 1, half random.
inline void fill(int dt, int op, size_t n, int which, uint64_t seed, unsigned char *out)
{
    const size_t es = esize(dt);
    const uint64_t m = mask_of(dt), top = 1ull << (8 * es - 1);
    const uint64_t sp[] = {0, 1, 2, 3, top - 1, top, top + 1, m - 1, m, 0x10, 0x0f, m >> 4, 0x55 & m, 0xaa & m};
    const uint64_t first[2][5] = {
        // x: all ones, top bit alone, largest positive, 2, a low half of ones
        {m, top, top - 1, 2, (1ull << (4 * es)) | 1},
        // y: 1 / all ones / 1 / 4 (no bit in common with 2) / the same low half
        {1, m, 1, 4, (1ull << (4 * es)) | 1}};
    for (size_t i = 0; i < n; i++) {
        uint64_t v;
        if (i < 5 && which < 2) {
            v = first[which][i];
            if (op == kProd && i == 0) v = m;          // all ones squared: 1 modulo 2^w, upper half all but full
            if (op == kProd && i == 2) v = which ? 3 : top - 1; // passes the signed range only
            if ((op == kLand || op == kLor || op == kLxor) && i == 1) v = which ? 0 : 2; // true against false
        } else {
            const uint64_t h = mix(seed ^ mix(((uint64_t)which << 40) ^ i));
            v = (h & 1) ? sp[(h >> 1) % (sizeof(sp) / sizeof(sp[0]))] : (h >> 8);
        }
        put(out + i * es, es, v & m);
    }
}

typedef std::vector<unsigned char> Bytes;

// The lengths of every GPU case: scalar only; head + tail and no body; one full 16 KiB tile, one
// partial tile and a tail (in elements of `es` bytes)
inline std::vector<size_t> case_lengths(size_t es) { return {5, 31, (16384 + 16) / es + 3}; }
inline uint64_t case_seed(int dt, int op, size_t n) { return mix(((uint64_t)dt << 32) ^ ((uint64_t)op << 24) ^ n); }

} // namespace iref
