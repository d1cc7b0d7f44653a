// TEST-ONLY, host-only: a plain reference of one reduction step, inout = inout op in, for the
// element types the oracle does not know -- float16, bfloat16 and MPI's three pair types.  The
// four types the oracle has are passed on to ftar_oracle_reduce_local.
//
// Nothing here is shared with the product's kernels, and no _Float16 / __bf16 arithmetic is
// used: a 16-bit element is decoded to double by its fields, SUM / PROD are ONE double operation
// rounded ONCE into the element format (nearest even, gradual underflow, overflow to infinity).
// That is the correctly rounded result: sums and products of two binary16 values and products of
// two bfloat16 values are exact in double, and a bfloat16 sum that is not exact has been rounded
// to 53 >= 2 * 8 + 2 significand bits, which makes the second rounding harmless.  MAX / MIN are
// (x > y) ? x : y and (x < y) ? x : y on the decoded values, x the in-out operand, the result the
// chosen operand's own 16 bits (a NaN on either side gives y).  Pairs follow include/ftar.h: x
// wins with the larger (MINLOC: smaller) value, or an equal value and the lower index; otherwise
// y, all bytes, padding included.  (tests/test_kernel_ref.py pins all of it against torch's CPU
// arithmetic and numpy.)
//
// `Round` other than kNearestEven gives deliberately WRONG roundings: the mutants that ref_check's
// selftest uses to show that the checkers' inputs can tell a wrong kernel from a right one.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

extern "C" int ftar_oracle_reduce_local(int dtype, int op, const void *in, void *inout, size_t n);

namespace kref {

// include/ftar.h's numbers (the checkers static_assert them against ftar_kernels.h)
enum { kInt32 = 0, kFloat32 = 1, kInt64 = 2, kFloat64 = 3, kFloat16 = 16, kBFloat16 = 17,
       kFloatInt = 32, k2Int = 33, kDoubleInt = 34 };
enum { kSum = 0, kProd = 1, kMax = 2, kMin = 3, kMaxloc = 16, kMinloc = 17 };
enum Round { kNearestEven = 0, kTowardZero = 1, kTiesAway = 2, kFlushSubnormal = 3 };

inline bool is16(int dt) { return dt == kFloat16 || dt == kBFloat16; }
inline bool is_pair(int dt) { return dt == kFloatInt || dt == k2Int || dt == kDoubleInt; }
inline size_t esize(int dt)
{
    if (is16(dt)) return 2;
    if (dt == kDoubleInt) return 16;
    if (dt == kFloatInt || dt == k2Int || dt == kInt64 || dt == kFloat64) return 8;
    return 4;
}

// the two 16-bit formats: mantissa bits, exponent bits
inline int mant_bits(int dt) { return dt == kFloat16 ? 10 : 7; }
inline int exp_bits(int dt) { return dt == kFloat16 ? 5 : 8; }

inline double pow2(int e) // 2^e, e in the normal range of double
{
    const uint64_t u = (uint64_t)(e + 1023) << 52;
    double d;
    memcpy(&d, &u, 8);
    return d;
}

inline double decode16(uint16_t b, int dt)
{
    const int mb = mant_bits(dt), eb = exp_bits(dt), bias = (1 << (eb - 1)) - 1;
    const int e = (b >> mb) & ((1 << eb) - 1), m = b & ((1 << mb) - 1);
    const double s = (b & 0x8000) ? -1.0 : 1.0;
    if (e == (1 << eb) - 1) {
        if (m) {
            const uint64_t q = 0x7ff8000000000000ull | ((uint64_t)(b >> 15) << 63);
            double d;
            memcpy(&d, &q, 8);
            return d;
        }
        const uint64_t q = 0x7ff0000000000000ull | ((uint64_t)(b >> 15) << 63);
        double d;
        memcpy(&d, &q, 8);
        return d;
    }
    if (e == 0) return s * (double)m * pow2(1 - bias - mb);
    return s * (double)((1 << mb) + m) * pow2(e - bias - mb);
}

// one rounding of a double into the element format
inline uint16_t encode16(double v, int dt, Round mode = kNearestEven)
{
    const int mb = mant_bits(dt), eb = exp_bits(dt), bias = (1 << (eb - 1)) - 1, emax = bias, emin = 1 - bias;
    const uint16_t inf = (uint16_t)(((1 << eb) - 1) << mb);
    uint64_t u;
    memcpy(&u, &v, 8);
    const uint16_t sign = (uint16_t)((u >> 63) << 15);
    const int de = (int)((u >> 52) & 0x7ff);
    const uint64_t dm = u & ((1ull << 52) - 1);
    if (de == 0x7ff) return (uint16_t)(sign | inf | (dm ? 1 << (mb - 1) : 0));
    if (de == 0) return sign; // zero (a subnormal double is below half of either format's smallest subnormal)
    const int E = de - 1023;
    const uint64_t sig = dm | (1ull << 52); // |v| = sig * 2^(E - 52)
    int Eq = E < emin ? emin : E;           // the result's exponent: its quantum is 2^(Eq - mb)
    const int sh = (Eq - mb) - (E - 52);    // bits below the quantum, >= 52 - mb
    uint64_t k = 0, rem = 1, half = 2;      // sh >= 64: far below half a quantum, and not zero
    if (sh < 64) {
        k = sig >> sh;
        rem = sig & ((1ull << sh) - 1);
        half = 1ull << (sh - 1);
    }
    bool up;
    if (mode == kTowardZero) up = false;
    else if (mode == kTiesAway) up = rem >= half;
    else up = rem > half || (rem == half && (k & 1));
    k += up;
    if (k >> (mb + 1)) {
        k >>= 1;
        Eq++;
    }
    if (k < (1ull << mb)) return (uint16_t)(sign | (mode == kFlushSubnormal ? 0 : k)); // subnormal or zero
    if (Eq > emax) return (uint16_t)(sign | (mode == kTowardZero ? inf - 1 : inf));
    return (uint16_t)(sign | ((Eq + bias) << mb) | (k - (1ull << mb)));
}

inline uint16_t apply16(int dt, int op, uint16_t x, uint16_t y, Round mode)
{
    const double a = decode16(x, dt), b = decode16(y, dt);
    switch (op) {
    case kSum: return encode16(a + b, dt, mode);
    case kProd: return encode16(a * b, dt, mode);
    case kMax: return (a > b) ? x : y;
    default: return (a < b) ? x : y;
    }
}

template <typename V> inline bool loc_x_wins(int op, V xv, int32_t xi, V yv, int32_t yi)
{
    if (op == kMaxloc ? xv > yv : xv < yv) return true;
    return xv == yv && xi < yi;
}

// x, y: one element each; true when the result is x
inline bool pair_x_wins(int dt, int op, const unsigned char *x, const unsigned char *y)
{
    int32_t xi, yi;
    if (dt == kDoubleInt) {
        double xv, yv;
        memcpy(&xv, x, 8);
        memcpy(&yv, y, 8);
        memcpy(&xi, x + 8, 4);
        memcpy(&yi, y + 8, 4);
        return loc_x_wins(op, xv, xi, yv, yi);
    }
    memcpy(&xi, x + 4, 4);
    memcpy(&yi, y + 4, 4);
    if (dt == kFloatInt) {
        float xv, yv;
        memcpy(&xv, x, 4);
        memcpy(&yv, y, 4);
        return loc_x_wins(op, xv, xi, yv, yi);
    }
    int32_t xv, yv;
    memcpy(&xv, x, 4);
    memcpy(&yv, y, 4);
    return loc_x_wins(op, xv, xi, yv, yi);
}

// The oracle's operand roles: inout = inout op in.  0, or the oracle's / this file's refusal.
inline int reduce_local(int dt, int op, const void *in, void *inout, size_t n, Round mode = kNearestEven)
{
    if (is16(dt)) {
        if (op < kSum || op > kMin) return 9;
        const unsigned char *y = (const unsigned char *)in;
        unsigned char *x = (unsigned char *)inout;
        for (size_t i = 0; i < n; i++) {
            uint16_t a, b;
            memcpy(&a, x + 2 * i, 2);
            memcpy(&b, y + 2 * i, 2);
            a = apply16(dt, op, a, b, mode);
            memcpy(x + 2 * i, &a, 2);
        }
        return 0;
    }
    if (is_pair(dt)) {
        if (op != kMaxloc && op != kMinloc) return 9;
        const size_t es = esize(dt);
        const unsigned char *y = (const unsigned char *)in;
        unsigned char *x = (unsigned char *)inout;
        for (size_t i = 0; i < n; i++)
            if (!pair_x_wins(dt, op, x + i * es, y + i * es)) memcpy(x + i * es, y + i * es, es);
        return 0;
    }
    return ftar_oracle_reduce_local(dt, op, in, inout, n);
}

// true where an element of a 16-bit buffer is a NaN (the places compared by NaN-ness only)
inline bool is_nan16(uint16_t b, int dt)
{
    const int mb = mant_bits(dt);
    const uint16_t inf = (uint16_t)(((1 << exp_bits(dt)) - 1) << mb);
    return (b & inf) == inf && (b & ((1 << mb) - 1)) != 0;
}

} // namespace kref
