// ftar_kernels.hip -- CDNA4 (gfx950) kernels of the fault-tolerant Allreduce.
//
// Every kernel here is HBM- or xGMI-bound integer/float streaming work: one pass over
// the operands, no reuse, no MFMA.  What matters on MI355X:
//   * 16-byte lanes (global_load_dwordx4 / global_store_dwordx4): 1 KiB per wave
//     instruction, the widest coalesced access;
//   * enough bytes in flight and short-lived blocks: one 16 KiB tile per operand per
//     256-thread workgroup, four independent 16-byte non-temporal loads per lane and
//     operand, non-temporal stores, one tile per block (32768 workgroups for the 256 MiB
//     C2 reduce) -- the fastest mapping of the rotating-buffer sweep (tools/hbm_sweep.hip);
//   * one launch handles up to FDEV_MAX_KSEGS independent segments (e.g. Raben's
//     step 0: reduce half the window + copy the other half of the partner's vector),
//     blocks are split between segments in proportion to their bytes and each wave
//     finds its segment with a wave-uniform (readfirstlane) search;
//   * segments whose pointers are not co-aligned to 16 bytes are split by the host
//     into a scalar head, a vector body and a scalar tail.
// Peer (xGMI) pointers obtained through hipIpcOpenMemHandle are plain device pointers
// here: the same kernel is the local reduce and the fused "pull + reduce" exchange.
//
// Reference semantics restated: MPI_Reduce_local(in, inout) = inout <op> in with
// OpenMPI's operand roles (out = out + in; max: out = (out > in) ? out : in), see
// include/ftar.h.  int32/int64 SUM/PROD wrap (two's complement), floats are one IEEE
// op per element (-ffp-contract=off, no fast-math).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "ftar_kernels.h"

namespace ftar {

// ---------------------------------------------------------------------------------
// element ops
// ---------------------------------------------------------------------------------
template <typename T> struct Arith { using U = T; };
template <> struct Arith<int32_t> { using U = uint32_t; };
template <> struct Arith<int64_t> { using U = uint64_t; };
// The 8- and 16-bit integers: C promotes both operands to (signed) int, and 65535 * 65535
// overflows it -- undefined.  SUM / PROD are done in uint32_t and truncated: modulo 2^w.
template <> struct Arith<uint8_t> { using U = uint32_t; };
template <> struct Arith<int8_t> { using U = uint32_t; };
template <> struct Arith<uint16_t> { using U = uint32_t; };
template <> struct Arith<int16_t> { using U = uint32_t; };

// Element types instantiated for MAX / MIN only: within one width signed and unsigned give the
// same bits for every other op, which runs on the width's canonical type (canon_dtype,
// ftar_kernels.h: uint8_t, uint16_t, int32_t, int64_t).
template <typename T> struct is_order_only : std::false_type {};
template <> struct is_order_only<int8_t> : std::true_type {};
template <> struct is_order_only<int16_t> : std::true_type {};
template <> struct is_order_only<uint32_t> : std::true_type {};
template <> struct is_order_only<uint64_t> : std::true_type {};

// The 2-byte float types: plain bit containers (sizeof == 2 gives 8 elements per 16-byte
// vector); the arithmetic is in the apply / apply16 overloads below.
struct f16_t { uint16_t b; };
struct bf16_t { uint16_t b; };
static_assert(sizeof(f16_t) == 2 && sizeof(bf16_t) == 2, "2-byte elements");

template <typename T, int OP>
__device__ __forceinline__ T apply(T x, T y)
{
    using U = typename Arith<T>::U;
    if constexpr (OP == kSum) return (T)((U)x + (U)y);
    else if constexpr (OP == kProd) return (T)((U)x * (U)y);
    else if constexpr (OP == kMax) return (x > y) ? x : y;
    else if constexpr (OP == kMin) return (x < y) ? x : y;
    // MPI's logical and bitwise ops (integer types only; the logical ones give 0 / 1)
    else if constexpr (OP == kLand) return (T)((x != 0) && (y != 0));
    else if constexpr (OP == kBand) return (T)(x & y);
    else if constexpr (OP == kLor) return (T)((x != 0) || (y != 0));
    else if constexpr (OP == kBor) return (T)(x | y);
    else if constexpr (OP == kLxor) return (T)((x != 0) != (y != 0));
    else return (T)(x ^ y);
}

// float16: the arithmetic is the hardware's own binary16 (v_add_f16 / v_mul_f16: one
// correctly rounded IEEE operation, subnormals kept -- the f16 denormal mode is on).  MAX /
// MIN are compare-and-select like every other type: the result is one of the two operands
// bit for bit (v_max_f16 / v_min_f16 would return +0 or -0 by their own rule and quiet a NaN).
template <int OP>
__device__ __forceinline__ f16_t apply_f16(f16_t x, f16_t y)
{
    _Float16 a, b;
    __builtin_memcpy(&a, &x, 2);
    __builtin_memcpy(&b, &y, 2);
    if constexpr (OP == kSum) a = a + b;
    else if constexpr (OP == kProd) a = a * b;
    else if constexpr (OP == kMax) return (a > b) ? x : y;
    else return (a < b) ? x : y;
    f16_t r;
    __builtin_memcpy(&r, &a, 2);
    return r;
}
template <> __device__ __forceinline__ f16_t apply<f16_t, kSum>(f16_t x, f16_t y) { return apply_f16<kSum>(x, y); }
template <> __device__ __forceinline__ f16_t apply<f16_t, kProd>(f16_t x, f16_t y) { return apply_f16<kProd>(x, y); }
template <> __device__ __forceinline__ f16_t apply<f16_t, kMax>(f16_t x, f16_t y) { return apply_f16<kMax>(x, y); }
template <> __device__ __forceinline__ f16_t apply<f16_t, kMin>(f16_t x, f16_t y) { return apply_f16<kMin>(x, y); }

// bfloat16: widened to float32 (exact: the 16 bits are the float's upper half), one float32
// operation, rounded once to nearest even (v_cvt_pk_bf16_f32 on gfx950).  The float32 result
// of a SUM or PROD of two bfloat16 values carries 24 >= 2 * 8 + 2 significand bits, so the
// second rounding gives the correctly rounded bfloat16 result.  MAX / MIN compare the widened
// values and return the chosen operand's own bits.
__device__ __forceinline__ float bf16_widen(bf16_t v) { return __builtin_bit_cast(float, (uint32_t)v.b << 16); }
template <int OP>
__device__ __forceinline__ bf16_t apply_bf16(bf16_t x, bf16_t y)
{
    const float a = bf16_widen(x), b = bf16_widen(y);
    if constexpr (OP == kMax) return (a > b) ? x : y;
    else if constexpr (OP == kMin) return (a < b) ? x : y;
    else {
        const __bf16 r = (__bf16)(OP == kSum ? a + b : a * b);
        return bf16_t{__builtin_bit_cast(uint16_t, r)};
    }
}
template <> __device__ __forceinline__ bf16_t apply<bf16_t, kSum>(bf16_t x, bf16_t y) { return apply_bf16<kSum>(x, y); }
template <> __device__ __forceinline__ bf16_t apply<bf16_t, kProd>(bf16_t x, bf16_t y) { return apply_bf16<kProd>(x, y); }
template <> __device__ __forceinline__ bf16_t apply<bf16_t, kMax>(bf16_t x, bf16_t y) { return apply_bf16<kMax>(x, y); }
template <> __device__ __forceinline__ bf16_t apply<bf16_t, kMin>(bf16_t x, bf16_t y) { return apply_bf16<kMin>(x, y); }

// MPI's pair types (value, index): plain element structs of 8, 8 and 16 bytes with the
// alignment of their C layout (4, 4, 8), the 16-byte one with its padding named so that a copy
// of the struct carries it.  MAXLOC / MINLOC only: compare-and-select of whole elements.
struct fi_t { float v; int32_t i; };
struct ii_t { int32_t v; int32_t i; };
struct di_t { double v; int32_t i; uint32_t pad; };
static_assert(sizeof(fi_t) == 8 && alignof(fi_t) == 4 && sizeof(ii_t) == 8 && alignof(ii_t) == 4, "8-byte pairs");
static_assert(sizeof(di_t) == 16 && alignof(di_t) == 8, "MPI_DOUBLE_INT, LP64");
template <typename T> struct is_pair : std::false_type {};
template <> struct is_pair<fi_t> : std::true_type {};
template <> struct is_pair<ii_t> : std::true_type {};
template <> struct is_pair<di_t> : std::true_type {};

// x wins: the larger (MAXLOC) or smaller (MINLOC) value, an equal value with the lower index.
// A NaN value fails every comparison: y.  The three compares are combined as lane masks (| and
// &, not || and &&: nothing to short-circuit, and no branch around a compare).
template <int OP, typename V>
__device__ __forceinline__ bool loc_takes_x(V xv, int32_t xi, V yv, int32_t yi)
{
    static_assert(OP == kMaxloc || OP == kMinloc, "pair types have MAXLOC / MINLOC only");
    const bool better = OP == kMaxloc ? xv > yv : xv < yv;
    return better | ((xv == yv) & (xi < yi));
}
#define FTAR_APPLY_LOC(T, OP)                                                                                  \
    template <> __device__ __forceinline__ T apply<T, OP>(T x, T y) { return loc_takes_x<OP>(x.v, x.i, y.v, y.i) ? x : y; }
FTAR_APPLY_LOC(fi_t, kMaxloc)
FTAR_APPLY_LOC(fi_t, kMinloc)
FTAR_APPLY_LOC(ii_t, kMaxloc)
FTAR_APPLY_LOC(ii_t, kMinloc)
FTAR_APPLY_LOC(di_t, kMaxloc)
FTAR_APPLY_LOC(di_t, kMinloc)
#undef FTAR_APPLY_LOC

// Runs fn(std::integral_constant<int, OP>) for the runtime op: one instantiation per op
// the element type has (the logical / bitwise ops only for the integer types, MAXLOC /
// MINLOC and nothing else for the pair types, MAX / MIN and nothing else for the order-only
// integer types).
template <typename T, typename Fn>
static hipError_t with_op(int op, Fn &&fn)
{
    using std::integral_constant;
    if constexpr (is_pair<T>::value) {
        switch (op) {
        case kMaxloc: return fn(integral_constant<int, kMaxloc>{});
        case kMinloc: return fn(integral_constant<int, kMinloc>{});
        default: return hipErrorInvalidValue;
        }
    } else if constexpr (is_order_only<T>::value) {
        switch (op) {
        case kMax: return fn(integral_constant<int, kMax>{});
        case kMin: return fn(integral_constant<int, kMin>{});
        default: return hipErrorInvalidValue;
        }
    } else {
        switch (op) {
        case kSum: return fn(integral_constant<int, kSum>{});
        case kProd: return fn(integral_constant<int, kProd>{});
        case kMax: return fn(integral_constant<int, kMax>{});
        case kMin: return fn(integral_constant<int, kMin>{});
        default: break;
        }
        if constexpr (std::is_integral<T>::value) {
            switch (op) {
            case kLand: return fn(integral_constant<int, kLand>{});
            case kBand: return fn(integral_constant<int, kBand>{});
            case kLor: return fn(integral_constant<int, kLor>{});
            case kBor: return fn(integral_constant<int, kBor>{});
            case kLxor: return fn(integral_constant<int, kLxor>{});
            case kBxor: return fn(integral_constant<int, kBxor>{});
            default: break;
            }
        }
        return hipErrorInvalidValue;
    }
}

// Runs fn(type_tag<T>) for the runtime dtype: T is the element type whose instantiation computes
// `op` on `dtype` (canon_dtype, ftar_kernels.h).  The one dtype switch of the launchers below;
// with_op<T> inside fn then picks the op.
template <typename T> struct type_tag { using type = T; };
template <typename Fn>
static hipError_t with_type(int dtype, int op, Fn &&fn)
{
    switch (canon_dtype(dtype, op)) {
    case kInt32: return fn(type_tag<int32_t>{});
    case kFloat32: return fn(type_tag<float>{});
    case kInt64: return fn(type_tag<int64_t>{});
    case kFloat64: return fn(type_tag<double>{});
    case kFloat16: return fn(type_tag<f16_t>{});
    case kBFloat16: return fn(type_tag<bf16_t>{});
    case kFloatInt: return fn(type_tag<fi_t>{});
    case k2Int: return fn(type_tag<ii_t>{});
    case kDoubleInt: return fn(type_tag<di_t>{});
    case kInt8: return fn(type_tag<int8_t>{});
    case kUInt8: return fn(type_tag<uint8_t>{});
    case kInt16: return fn(type_tag<int16_t>{});
    case kUInt16: return fn(type_tag<uint16_t>{});
    case kUInt32: return fn(type_tag<uint32_t>{});
    case kUInt64: return fn(type_tag<uint64_t>{});
    default: return hipErrorInvalidValue;
    }
}

// The 8- and 16-bit integers' vector path, one 32-bit register (two or four elements) at a time.
// gfx950 has packed 16-bit integer add, mul_lo, max, min and shifts (v_pk_*_u16 / _i16, reached
// through ext_vector_type arithmetic and the elementwise builtins) and no packed 8-bit ALU at all:
// the generic per-element loop unpacks every byte (v_bfe / v_lshrrev), combines it and packs the
// results again (v_perm / v_lshl_or).  The forms below are the same functions of the bits:
//   bitwise ops        whole-register logic, whatever the width;
//   logical ops        per element "any bit set" as 0 / 1 -- 16-bit: min(x, 1) unsigned; 8-bit:
//                      SWAR, bit 7 of (low 7 bits + 0x7f) | x moved down -- then and / or / xor
//                      (LOR: one "any bit set" of x | y);
//   16-bit arithmetic  the packed ops themselves (unsigned vector arithmetic wraps: no promotion
//                      to int takes place on vector operands);
//   8-bit SUM          carry-isolating SWAR: the low 7 bits of every byte added with bit 7 clear
//                      (no carry leaves a byte), bit 7 put back as the xor of the operands' and
//                      the carry into it;
//   8-bit PROD         even and odd bytes through the packed 16-bit multiply.  The low byte of a
//                      product depends on the operands' low bytes only (even bytes: a as loaded);
//                      (a_odd << 8) * b_odd is the product's low byte in the odd position already;
//                      one v_perm_b32 takes the even bytes of the one and the odd bytes of the other;
//   8-bit MAX / MIN    even and odd bytes through the packed 16-bit max / min with the byte in
//                      the HIGH half of its 16-bit lane, where the lane's own signedness is the
//                      byte's.  Odd bytes: the operands as loaded -- a 16-bit lane orders by its
//                      high byte first, so the high byte of the lane's max IS the max of the high
//                      bytes, whatever the low bytes did.  Even bytes: shifted up by 8.  One
//                      v_perm_b32 puts the four high bytes in place.  An integer max is one of its
//                      operands, so this is (x > y) ? x : y bit for bit.
typedef unsigned short us2_t __attribute__((ext_vector_type(2)));
typedef short ss2_t __attribute__((ext_vector_type(2)));
template <typename T> struct is_narrow_int : std::integral_constant<bool, std::is_integral<T>::value && sizeof(T) <= 2> {};

template <int OP, typename V>
__device__ __forceinline__ uint32_t pk_order16(uint32_t a, uint32_t b)
{
    const V x = __builtin_bit_cast(V, a), y = __builtin_bit_cast(V, b);
    return __builtin_bit_cast(uint32_t, OP == kMax ? __builtin_elementwise_max(x, y) : __builtin_elementwise_min(x, y));
}
__device__ __forceinline__ uint32_t pk_mul16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2_t, a) * __builtin_bit_cast(us2_t, b));
}
__device__ __forceinline__ uint32_t pk_shl16(uint32_t a, int k)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2_t, a) << (us2_t)(unsigned short)k);
}
__device__ __forceinline__ uint32_t pk_shr16(uint32_t a, int k)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2_t, a) >> (us2_t)(unsigned short)k);
}
// per element 1 where any bit is set, else 0
__device__ __forceinline__ uint32_t nz16(uint32_t a) { return pk_order16<kMin, us2_t>(a, 0x00010001u); }
__device__ __forceinline__ uint32_t nz8(uint32_t a)
{
    return ((((a & 0x7f7f7f7fu) + 0x7f7f7f7fu) | a) >> 7) & 0x01010101u;
}

template <typename T, int OP>
__device__ __forceinline__ uint32_t pk_int(uint32_t a, uint32_t b)
{
    constexpr bool k8 = sizeof(T) == 1;
    constexpr uint32_t kEven = 0x00ff00ffu, kOdd = 0xff00ff00u;
    // v_perm_b32 selectors (byte i of the result: 0..3 = byte of the second source, 4..7 = of the first)
    constexpr uint32_t kOddOfFirstEvenOfSecond = 0x07020500u; // {first.3, second.2, first.1, second.0}
    constexpr uint32_t kHighBytesInterleaved = 0x07030501u;   // {first.3, second.3, first.1, second.1}
    if constexpr (OP == kBand) return a & b;
    else if constexpr (OP == kBor) return a | b;
    else if constexpr (OP == kBxor) return a ^ b;
    else if constexpr (OP == kLand) return k8 ? nz8(a) & nz8(b) : nz16(a) & nz16(b);
    else if constexpr (OP == kLor) return k8 ? nz8(a | b) : nz16(a | b);
    else if constexpr (OP == kLxor) return k8 ? nz8(a) ^ nz8(b) : nz16(a) ^ nz16(b);
    else if constexpr (OP == kSum) {
        if constexpr (k8) return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u);
        else return __builtin_bit_cast(uint32_t, __builtin_bit_cast(us2_t, a) + __builtin_bit_cast(us2_t, b));
    } else if constexpr (OP == kProd) {
        if constexpr (k8)
            return __builtin_amdgcn_perm(pk_mul16(a & kOdd, pk_shr16(b, 8)), pk_mul16(a, b & kEven), kOddOfFirstEvenOfSecond);
        else return pk_mul16(a, b);
    } else { // MAX / MIN in the type's own signedness
        using V = typename std::conditional<std::is_signed<T>::value, ss2_t, us2_t>::type;
        if constexpr (k8)
            return __builtin_amdgcn_perm(pk_order16<OP, V>(a, b), pk_order16<OP, V>(pk_shl16(a, 8), pk_shl16(b, 8)),
                                         kHighBytesInterleaved);
        else return pk_order16<OP, V>(a, b);
    }
}

template <typename T, int OP>
__device__ __forceinline__ uint4 apply16(uint4 a, uint4 b)
{
    if constexpr (is_narrow_int<T>::value)
        return make_uint4(pk_int<T, OP>(a.x, b.x), pk_int<T, OP>(a.y, b.y), pk_int<T, OP>(a.z, b.z), pk_int<T, OP>(a.w, b.w));
    constexpr int E = 16 / sizeof(T);
    T xa[E], xb[E];
    __builtin_memcpy(xa, &a, 16);
    __builtin_memcpy(xb, &b, 16);
#pragma unroll
    for (int e = 0; e < E; e++) xa[e] = apply<T, OP>(xa[e], xb[e]);
    uint4 r;
    __builtin_memcpy(&r, xa, 16);
    return r;
}

// The 16-bit types' vector path, two elements per 32-bit register.
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef float f2_t __attribute__((ext_vector_type(2)));
typedef __bf16 b2_t __attribute__((ext_vector_type(2)));

// SUM / PROD of float16 pairs: packed binary16 math (v_pk_add_f16 / v_pk_mul_f16)
template <int OP>
__device__ __forceinline__ uint32_t pk_f16(uint32_t a, uint32_t b)
{
    const h2_t x = __builtin_bit_cast(h2_t, a), y = __builtin_bit_cast(h2_t, b);
    return __builtin_bit_cast(uint32_t, OP == kSum ? x + y : x * y);
}
// SUM / PROD of bfloat16 pairs: the low element widened by a shift, the high one by a mask,
// packed float32 math (v_pk_add_f32 / v_pk_mul_f32), one packed conversion back
template <int OP>
__device__ __forceinline__ uint32_t pk_bf16(uint32_t a, uint32_t b)
{
    const f2_t x = {__builtin_bit_cast(float, a << 16), __builtin_bit_cast(float, a & 0xffff0000u)};
    const f2_t y = {__builtin_bit_cast(float, b << 16), __builtin_bit_cast(float, b & 0xffff0000u)};
    const f2_t r = OP == kSum ? x + y : x * y;
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(r, b2_t));
}
// MAX / MIN of a pair: each half selected whole from a or b
template <typename T, int OP>
__device__ __forceinline__ uint32_t pk_sel(uint32_t a, uint32_t b)
{
    const T lo = apply<T, OP>(T{(uint16_t)a}, T{(uint16_t)b});
    const T hi = apply<T, OP>(T{(uint16_t)(a >> 16)}, T{(uint16_t)(b >> 16)});
    return (uint32_t)lo.b | ((uint32_t)hi.b << 16);
}
template <typename T, int OP>
__device__ __forceinline__ uint32_t pk16(uint32_t a, uint32_t b)
{
    if constexpr (OP == kMax || OP == kMin) return pk_sel<T, OP>(a, b);
    else if constexpr (std::is_same<T, f16_t>::value) return pk_f16<OP>(a, b);
    else return pk_bf16<OP>(a, b);
}
#define FTAR_APPLY16_PK(T, OP)                                                                                 \
    template <> __device__ __forceinline__ uint4 apply16<T, OP>(uint4 a, uint4 b)                              \
    {                                                                                                          \
        return make_uint4(pk16<T, OP>(a.x, b.x), pk16<T, OP>(a.y, b.y), pk16<T, OP>(a.z, b.z),                 \
                          pk16<T, OP>(a.w, b.w));                                                              \
    }
FTAR_APPLY16_PK(f16_t, kSum)
FTAR_APPLY16_PK(f16_t, kProd)
FTAR_APPLY16_PK(f16_t, kMax)
FTAR_APPLY16_PK(f16_t, kMin)
FTAR_APPLY16_PK(bf16_t, kSum)
FTAR_APPLY16_PK(bf16_t, kProd)
FTAR_APPLY16_PK(bf16_t, kMax)
FTAR_APPLY16_PK(bf16_t, kMin)
#undef FTAR_APPLY16_PK

// The pair types' vector path: the compare reads the value and index dwords where they were
// loaded, and every dword of the result is selected whole from a or b by it (v_cndmask_b32) --
// two independent selects per vector for the 8-byte types, one for the 16-byte type, whose
// padding dword travels like the others.
__device__ __forceinline__ float pair_val(const fi_t *, uint32_t v) { return __builtin_bit_cast(float, v); }
__device__ __forceinline__ int32_t pair_val(const ii_t *, uint32_t v) { return (int32_t)v; }
#define FTAR_APPLY16_LOC8(T, OP)                                                                               \
    template <> __device__ __forceinline__ uint4 apply16<T, OP>(uint4 a, uint4 b)                              \
    {                                                                                                          \
        constexpr const T *tag = nullptr;                                                                      \
        const bool t0 = loc_takes_x<OP>(pair_val(tag, a.x), (int32_t)a.y, pair_val(tag, b.x), (int32_t)b.y);   \
        const bool t1 = loc_takes_x<OP>(pair_val(tag, a.z), (int32_t)a.w, pair_val(tag, b.z), (int32_t)b.w);   \
        return make_uint4(t0 ? a.x : b.x, t0 ? a.y : b.y, t1 ? a.z : b.z, t1 ? a.w : b.w);                     \
    }
FTAR_APPLY16_LOC8(fi_t, kMaxloc)
FTAR_APPLY16_LOC8(fi_t, kMinloc)
FTAR_APPLY16_LOC8(ii_t, kMaxloc)
FTAR_APPLY16_LOC8(ii_t, kMinloc)
#undef FTAR_APPLY16_LOC8
#define FTAR_APPLY16_LOC16(OP)                                                                                 \
    template <> __device__ __forceinline__ uint4 apply16<di_t, OP>(uint4 a, uint4 b)                           \
    {                                                                                                          \
        const double av = __builtin_bit_cast(double, (uint64_t)a.x | ((uint64_t)a.y << 32));                   \
        const double bv = __builtin_bit_cast(double, (uint64_t)b.x | ((uint64_t)b.y << 32));                   \
        const bool t = loc_takes_x<OP>(av, (int32_t)a.z, bv, (int32_t)b.z);                                    \
        return make_uint4(t ? a.x : b.x, t ? a.y : b.y, t ? a.z : b.z, t ? a.w : b.w);                         \
    }
FTAR_APPLY16_LOC16(kMaxloc)
FTAR_APPLY16_LOC16(kMinloc)
#undef FTAR_APPLY16_LOC16

// ---------------------------------------------------------------------------------
// segment kernel
// ---------------------------------------------------------------------------------
// (kBlock threads per workgroup, kUnroll vectors per lane and operand: ftar_kernels.h)

// Streaming operands are read once and results are not re-read by this kernel:
// non-temporal loads AND stores (global_load/store_dwordx4 ... nt).  Timed on rotating
// buffers (tools/hbm_sweep.hip: every launch on one of 4 pairs, 2 GiB, so the 256 MiB
// Infinity Cache holds nothing the next launch reads) the C2 reduce runs at 6.2 TB/s
// with nt stores against 5.6 TB/s with plain ones.  (Round 1's sweep looped over ONE
// pair: there plain stores left the result in the Infinity Cache for the next launch to
// read, which made them look faster -- an artefact of the benchmark, profiles/r02.)
// `nts` is uniform over the launch (FTAR_NT_STORE, default on).
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ldnt(const uint4 *p)
{
    v4u v = __builtin_nontemporal_load((const v4u *)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st16(uint4 *p, uint4 v, unsigned nts)
{
    if (nts) {
        v4u w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, (v4u *)p);
    } else {
        *p = v;
    }
}

// KSignal (ftar_kernels.h): optional acquire before the first load, release + completion
// flag after the last store.  The branch is uniform over the launch.
__device__ __forceinline__ void signal_acquire(const KSignal &G)
{
    if ((G.cnt || G.gate) && G.acquire) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, ""); // system scope: drop cached remote lines
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

// Staging phase of a gated launch (KSignal stage_*): this rank's input copied into its
// exported buffer, element by element (any alignment; a small launch), then released and
// signalled to the host -- all before the gate, which the host opens only after it saw the
// signal and the peers' barrier.  The grid is small (<= FTAR_FLAG_MAX_BLOCKS workgroups), so
// every workgroup is resident while the others wait at the gate.
template <typename E>
__device__ __forceinline__ void stage_copy(const KSignal &G, size_t n)
{
    const E *s = (const E *)G.stage_src;
    E *d = (E *)G.stage_dst;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) d[i] = s[i];
}

// 16-byte vectors when both ends are 16-byte aligned (the workspace and a hipMalloc'd input
// are), the elements past the last whole vector one by one
__device__ __forceinline__ bool stage_copy_vec(const KSignal &G)
{
    if ((((uintptr_t)G.stage_src | (uintptr_t)G.stage_dst) & 15) != 0) return false;
    const size_t nv = G.stage_n * G.stage_es / 16;
    const uint4 *s = (const uint4 *)G.stage_src;
    uint4 *d = (uint4 *)G.stage_dst;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) d[i] = s[i];
    const size_t done = nv * 16 / G.stage_es; // elements copied as vectors (all of them at 16 bytes each)
    if (blockIdx.x == 0)
        for (size_t i = done + threadIdx.x; i < G.stage_n; i += blockDim.x) {
            if (G.stage_es == 8) ((unsigned long long *)G.stage_dst)[i] = ((const unsigned long long *)G.stage_src)[i];
            else if (G.stage_es == 2) ((unsigned short *)G.stage_dst)[i] = ((const unsigned short *)G.stage_src)[i];
            else if (G.stage_es == 1) ((unsigned char *)G.stage_dst)[i] = ((const unsigned char *)G.stage_src)[i];
            else ((unsigned *)G.stage_dst)[i] = ((const unsigned *)G.stage_src)[i];
        }
    return true;
}

__device__ __forceinline__ void signal_stage(const KSignal &G)
{
    if (!G.stage_dst) return;
    if (stage_copy_vec(G)) {
    } else if (G.stage_es == 16) stage_copy<unsigned long long>(G, 2 * G.stage_n); // 8-byte aligned: two halves
    else if (G.stage_es == 8) stage_copy<unsigned long long>(G, G.stage_n);
    else if (G.stage_es == 2) stage_copy<unsigned short>(G, G.stage_n);
    else if (G.stage_es == 1) stage_copy<unsigned char>(G, G.stage_n);
    else stage_copy<unsigned>(G, G.stage_n);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, ""); // system scope: the staged input to HBM for the peers
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned old = __hip_atomic_fetch_add(G.stage_cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == gridDim.x - 1) {
            __hip_atomic_store(G.stage_cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(G.flag, G.stage_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// The gate of a launch queued ahead of its barrier (KSignal): 1 = run, 0 = skip.  One
// lane polls the host word with system-scope loads (uncached, over PCIe), sleeping
// between polls; the workgroup learns the verdict through LDS.  Uniform over the launch.
// Gates take turns over kGateSlots words (ftar_kernels.h): a workgroup that starts late
// still finds its own verdict after the host has opened the next gate.
// Thread 0: wait until `word` (scope S) reaches the gate's value; skip (and report) past
// `ticks` of the wall clock, or when the word already holds a later gate.
template <int S>
__device__ __forceinline__ unsigned gate_wait(const KSignal &G, const unsigned *word, unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    unsigned v;
    for (;;) {
        v = __hip_atomic_load(word, __ATOMIC_RELAXED, S);
        if ((int)((v & ~1u) - (G.gate_val & ~1u)) >= 0) break;
        if (wall_clock64() - t0 > ticks) { // the host never opened it: skip, report
            __hip_atomic_store(G.err, G.gate_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            v = G.gate_val | 1u;
            break;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    if ((v & ~1u) != G.gate_val) { // the slot already holds a later gate: never run blind
        __hip_atomic_store(G.err, G.gate_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        v |= 1u;
    }
    return v;
}

__device__ __forceinline__ bool signal_gate(const KSignal &G)
{
    if (G.vword) { // behind a peer wait: its verdict is in device memory already (stream order)
        __shared__ unsigned vgo;
        if (threadIdx.x == 0) vgo = __hip_atomic_load(G.vword, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G.vval;
        __syncthreads();
        if (!vgo) return false;
    }
    if (!G.gate) return true;
    __shared__ unsigned go;
    if (threadIdx.x == 0) {
        unsigned v;
        if (!G.gate_dev) {
            v = gate_wait<__HIP_MEMORY_SCOPE_SYSTEM>(G, G.gate, G.gate_ticks);
        } else {
            // relayed: the first workgroup of this gate polls the host word (over PCIe) and
            // relays the verdict through device memory; the others poll that (agent scope)
            const unsigned old = __hip_atomic_fetch_max(G.gate_poll, G.gate_val, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
            if ((int)(old - G.gate_val) < 0) {
                v = gate_wait<__HIP_MEMORY_SCOPE_SYSTEM>(G, G.gate, G.gate_ticks);
                __hip_atomic_store(G.gate_dev, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                v = gate_wait<__HIP_MEMORY_SCOPE_AGENT>(G, G.gate_dev, 2 * G.gate_ticks);
            }
        }
        go = (v & 1u) ? 0u : 1u;
    }
    __syncthreads();
    return go != 0;
}

__device__ __forceinline__ void signal_done(const KSignal &G)
{
    if (!G.cnt) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's stores have completed
    __syncthreads();                                  // ... and every other wave's
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, ""); // system scope: this XCD's dirty lines to HBM
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the write-back completed (never elided)
        const unsigned old = __hip_atomic_fetch_add(G.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == gridDim.x - 1) { // every workgroup has released: the launch is done
            __hip_atomic_store(G.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(G.flag, G.tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <typename T, int OP>
__device__ __forceinline__ void vec_body(const KSeg &S, size_t b, size_t nblk, unsigned nts)
{
    // Block-contiguous tiles of kBlock * kUnroll vectors (16 KiB per operand per block):
    // each lane issues kUnroll independent 16-byte non-temporal loads per operand, wave
    // instructions stay 1 KiB coalesced, and the grid is sized so that one tile per block
    // covers the segment (the loop only runs when the host capped the grid).
    constexpr size_t E = 16 / sizeof(T);
    constexpr size_t kTile = (size_t)kBlock * kUnroll;
    const uint4 *__restrict__ X = (const uint4 *)S.x;
    const uint4 *__restrict__ Y = (const uint4 *)S.y;
    uint4 *__restrict__ O = (uint4 *)S.out;
    uint4 *__restrict__ O2 = (uint4 *)S.out2; // wave-uniform: both stores or one
    const size_t nv = S.n / E;
    for (size_t base = b * kTile; base < nv; base += nblk * kTile) {
        const size_t i = base + threadIdx.x;
        if (base + kTile <= nv) {
            uint4 a[kUnroll], c[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) a[u] = ldnt(X + i + u * kBlock);
            if (S.kind != kCopy) {
#pragma unroll
                for (int u = 0; u < kUnroll; u++) c[u] = ldnt(Y + i + u * kBlock);
#pragma unroll
                for (int u = 0; u < kUnroll; u++) a[u] = apply16<T, OP>(a[u], c[u]);
            }
#pragma unroll
            for (int u = 0; u < kUnroll; u++) st16(O + i + u * kBlock, a[u], nts);
            if (O2) {
#pragma unroll
                for (int u = 0; u < kUnroll; u++) st16(O2 + i + u * kBlock, a[u], nts);
            }
        } else {
            for (size_t j = i; j < nv; j += kBlock) {
                const uint4 xv = ldnt(X + j);
                const uint4 v = (S.kind == kCopy) ? xv : apply16<T, OP>(xv, ldnt(Y + j));
                st16(O + j, v, nts);
                if (O2) st16(O2 + j, v, nts);
            }
        }
    }
}

template <typename T, int OP>
__device__ __forceinline__ void scalar_body(const KSeg &S, size_t b, size_t nblk)
{
    const T *X = (const T *)S.x;
    const T *Y = (const T *)S.y;
    T *O = (T *)S.out;
    T *O2 = (T *)S.out2;
    const size_t stride = nblk * kBlock;
    for (size_t i = b * kBlock + threadIdx.x; i < S.n; i += stride) {
        const T xv = X[i];
        const T v = (S.kind == kCopy) ? xv : apply<T, OP>(xv, Y[i]);
        O[i] = v;
        if (O2) O2[i] = v;
    }
}

template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void segment_kernel(KSegList L)
{
    // blockIdx is wave-uniform; readfirstlane keeps the lookup in SGPRs.
    const unsigned b = (unsigned)__builtin_amdgcn_readfirstlane((int)blockIdx.x);
    const BlockWork w = map_block(L, b);
    const KSeg &S = L.s[__builtin_amdgcn_readfirstlane(w.seg)];
    signal_stage(L.sig);
    if (signal_gate(L.sig)) {
        signal_acquire(L.sig);
        if (S.vec) vec_body<T, OP>(S, w.first, w.stride, L.nt_store);
        else scalar_body<T, OP>(S, w.first, w.stride);
    }
    signal_done(L.sig);
}

// LDS-DMA staged local reduce (variant 1): the `in` operand is moved HBM -> LDS by
// global_load_lds_dwordx4 (no VGPR destination; 1 KiB per wave instruction, landing at
// the wave-uniform LDS base + 16 B x lane), the `inout` operand comes to VGPRs with
// plain dwordx4 loads issued meanwhile.  Each wave reads back only what it staged, so
// the only ordering needed is the wave's own vmcnt(0) -- no workgroup barrier.
template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void reduce_lds_kernel(uint4 *__restrict__ inout,
                                                            const uint4 *__restrict__ in, size_t nv, unsigned nts)
{
    __shared__ uint4 stage[kUnroll * kBlock]; // 16 KiB per workgroup (kUnroll = 4)
    const int wave = threadIdx.x >> 6;
    const size_t tile = (size_t)kUnroll * kBlock;
    for (size_t base = (size_t)blockIdx.x * tile; base < nv; base += (size_t)gridDim.x * tile) {
        uint4 a[kUnroll];
        if (base + tile <= nv) {
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const uint4 *g = in + base + (size_t)u * kBlock + threadIdx.x;
                uint4 *l = &stage[u * kBlock + wave * 64];
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                                 (__attribute__((address_space(3))) void *)l, 16, 0, 2 /* nt */);
            }
#pragma unroll
            for (int u = 0; u < kUnroll; u++) a[u] = ldnt(inout + base + (size_t)u * kBlock + threadIdx.x);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int u = 0; u < kUnroll; u++)
                st16(inout + base + (size_t)u * kBlock + threadIdx.x, apply16<T, OP>(a[u], stage[u * kBlock + threadIdx.x]),
                     nts);
        } else {
            for (size_t i = base + threadIdx.x; i < nv; i += kBlock) st16(inout + i, apply16<T, OP>(inout[i], in[i]), nts);
        }
    }
}

// Tree reduce over p sources (one-hop reduce-scatter on the xGMI mesh): every lane loads
// one 16-byte vector from each of the p sources -- p - 1 of them peers, so all links
// stream at once -- and combines them in the schedule's tree.  Workgroups past the
// vector body take the scalar head/tail (or everything, if the pointers are not
// co-aligned), grid-stride.
// U (1, 2, 4): 16-byte vectors per lane and source, every load of the workgroup's U x P
// vectors issued before the first combine -- more bytes in flight per lane when the
// sources are remote (xGMI load latency) rather than local HBM (FTAR_OPT_TREE_UNROLL; the
// node's transport selection times the forms).  Same tree per element: same bits.
template <typename T, int OP, int P>
__device__ __forceinline__ void tree_store(const TreeArgs &A, size_t i, uint4 (&v)[P])
{
#pragma unroll
    for (int w = 1; w < P; w <<= 1)
#pragma unroll
        for (int j = 0; j < P; j += 2 * w) v[j] = apply16<T, OP>(v[j], v[j + w]);
    st16((uint4 *)((T *)A.out + A.head) + i, v[0], A.nt_store);
    for (int o = 0; o < A.nmore; o++) st16((uint4 *)((T *)A.more[o] + A.head) + i, v[0], A.nt_store);
}

template <typename T, int OP, int P, int U>
__device__ __forceinline__ void tree_body(const TreeArgs &A, unsigned b, unsigned nblocks)
{
    if (b < A.nvb) {
        // chunk b, then b + nvb, ... (once, unless the planner capped the vector workgroups:
        // cap_tree_batch, a gated one-shot launch that must stay within the signal limit)
        for (size_t c = b; c * kBlock * U < A.nv; c += A.nvb) {
            const size_t i0 = c * kBlock * U + threadIdx.x;
            if (i0 + (size_t)(U - 1) * kBlock < A.nv) {
                uint4 v[U][P];
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int j = 0; j < P; j++)
                        v[u][j] = ldnt((const uint4 *)((const T *)A.src[j] + A.head) + i0 + (size_t)u * kBlock);
#pragma unroll
                for (int u = 0; u < U; u++) tree_store<T, OP, P>(A, i0 + (size_t)u * kBlock, v[u]);
            } else {
                for (int u = 0; u < U; u++) {
                    const size_t i = i0 + (size_t)u * kBlock;
                    if (i >= A.nv) break;
                    uint4 v[P];
#pragma unroll
                    for (int j = 0; j < P; j++) v[j] = ldnt((const uint4 *)((const T *)A.src[j] + A.head) + i);
                    tree_store<T, OP, P>(A, i, v);
                }
            }
        }
        return;
    }
    constexpr size_t E = 16 / sizeof(T);
    const size_t tail0 = A.head + A.nv * E; // scalar elements: [0, head) and [tail0, n)
    const size_t nscalar = A.head + (A.n - tail0);
    const size_t stride = (size_t)(nblocks - A.nvb) * kBlock;
    for (size_t k = (size_t)(b - A.nvb) * kBlock + threadIdx.x; k < nscalar; k += stride) {
        const size_t e = k < A.head ? k : tail0 + (k - A.head);
        T v[P];
#pragma unroll
        for (int j = 0; j < P; j++) v[j] = ((const T *)A.src[j])[e];
#pragma unroll
        for (int w = 1; w < P; w <<= 1)
#pragma unroll
            for (int j = 0; j < P; j += 2 * w) v[j] = apply<T, OP>(v[j], v[j + w]);
        ((T *)A.out)[e] = v[0];
        for (int o = 0; o < A.nmore; o++) ((T *)A.more[o])[e] = v[0];
    }
}

template <typename T, int OP, int P, int U>
__global__ __launch_bounds__(kBlock) void tree_kernel(TreeArgs A)
{
    tree_body<T, OP, P, U>(A, (unsigned)__builtin_amdgcn_readfirstlane((int)blockIdx.x), gridDim.x);
}

// Several trees in one launch (the one-shot mesh Allreduce: every block of the vector,
// each in its owner's tree): tree k takes workgroups [first[k], first[k + 1]).
template <typename T, int OP, int P>
__global__ __launch_bounds__(kBlock) void tree_batch_kernel(TreeBatch B)
{
    const unsigned b = (unsigned)__builtin_amdgcn_readfirstlane((int)blockIdx.x);
    int k = 0;
    while (k + 1 < B.nt && b >= B.first[k + 1]) k++;
    signal_stage(B.sig);
    if (signal_gate(B.sig)) {
        signal_acquire(B.sig);
        tree_body<T, OP, P, 1>(B.t[k], b - B.first[k], B.first[k + 1] - B.first[k]);
    }
    signal_done(B.sig);
}

// ---------------------------------------------------------------------------------
// host-side dispatch (the planners of these launches: ftar_plan.cpp)
// ---------------------------------------------------------------------------------
template <typename T, int OP, int P>
static void launch_tree_u(const TreeArgs &A, unsigned grid, hipStream_t s)
{
    if constexpr (P == 4 || P == 8) {
        if (A.unroll == 4) {
            hipLaunchKernelGGL((tree_kernel<T, OP, P, 4>), dim3(grid), dim3(kBlock), 0, s, A);
            return;
        }
        if (A.unroll == 2) {
            hipLaunchKernelGGL((tree_kernel<T, OP, P, 2>), dim3(grid), dim3(kBlock), 0, s, A);
            return;
        }
    }
    hipLaunchKernelGGL((tree_kernel<T, OP, P, 1>), dim3(grid), dim3(kBlock), 0, s, A);
}

template <typename T, int OP>
static hipError_t launch_tree_op(int p, const TreeArgs &A, unsigned grid, hipStream_t s)
{
    switch (p) {
    case 2: launch_tree_u<T, OP, 2>(A, grid, s); break;
    case 4: launch_tree_u<T, OP, 4>(A, grid, s); break;
    case 8: launch_tree_u<T, OP, 8>(A, grid, s); break;
    case 16: launch_tree_u<T, OP, 16>(A, grid, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_tree(int dtype, int op, int p, const TreeArgs &A, unsigned grid, hipStream_t s)
{
    return with_type(dtype, op, [&](auto t) {
        using T = typename decltype(t)::type;
        return with_op<T>(op, [&](auto o) { return launch_tree_op<T, decltype(o)::value>(p, A, grid, s); });
    });
}

template <typename T, int OP>
static hipError_t launch_batch_op(int p, const TreeBatch &B, unsigned grid, hipStream_t s)
{
    switch (p) {
    case 2: hipLaunchKernelGGL((tree_batch_kernel<T, OP, 2>), dim3(grid), dim3(kBlock), 0, s, B); break;
    case 4: hipLaunchKernelGGL((tree_batch_kernel<T, OP, 4>), dim3(grid), dim3(kBlock), 0, s, B); break;
    case 8: hipLaunchKernelGGL((tree_batch_kernel<T, OP, 8>), dim3(grid), dim3(kBlock), 0, s, B); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_tree_batch(int dtype, int op, int p, const TreeBatch &B, unsigned grid, hipStream_t s)
{
    return with_type(dtype, op, [&](auto t) {
        using T = typename decltype(t)::type;
        return with_op<T>(op, [&](auto o) { return launch_batch_op<T, decltype(o)::value>(p, B, grid, s); });
    });
}

// PeerWait (ftar_kernels.h): one wavefront, lane i < npeers polls peer i's flag.
__global__ __launch_bounds__(64) void peer_wait_kernel(PeerWait W)
{
    const int lane = threadIdx.x;
    if (lane == 0) {
        __hip_atomic_store(W.own, W.token, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, ""); // system scope: the flag out to host memory for the peers
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const unsigned long long *mine = lane < W.npeers ? W.peer[lane] : nullptr;
    const unsigned long long t0 = wall_clock64();
    bool go = false;
    for (;;) {
        const bool ready = !mine || __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= W.token;
        if (__all(ready)) {
            go = true;
            break;
        }
        if (__hip_atomic_load(W.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == W.vval) break;
        if (wall_clock64() - t0 > W.ticks) break;
        __builtin_amdgcn_s_sleep(2);
    }
    if (lane == 0) {
        const unsigned v = go ? W.vval : (W.vval | 1u);
        __hip_atomic_store(W.verdict_dev, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(W.verdict_host, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t launch_peer_wait(const PeerWait &W, hipStream_t s)
{
    if (W.npeers < 1 || W.npeers > kMaxPeers || !W.own || !W.abort_word || !W.verdict_dev || !W.verdict_host)
        return hipErrorInvalidValue;
    for (int i = 0; i < W.npeers; i++)
        if (!W.peer[i]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(peer_wait_kernel, dim3(1), dim3(64), 0, s, W);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// table-driven gather / scatter (GatherArgs, ftar_kernels.h)
// ---------------------------------------------------------------------------------
// User memory is streamed (read once on gather, not re-read by this rank on scatter):
// non-temporal.  The packed side is what the schedule reads next (gather: plain stores, a small
// call's staging copy or one-shot launch then finds them in cache) or has just written
// (scatter: plain loads).
// Both sides are global memory (device or mapped pinned host memory), which the compiler cannot
// see for pointers loaded from the table: said here, so that it emits global_* and not flat_*.
#define FTAR_GLOBAL __attribute__((address_space(1)))
template <bool SCATTER, typename U>
__device__ __forceinline__ void move_units(char *user, char *packed, size_t bytes, unsigned tid, unsigned nth)
{
    FTAR_GLOBAL U *u = (FTAR_GLOBAL U *)user, *k = (FTAR_GLOBAL U *)packed;
    const size_t n = bytes / sizeof(U);
    for (size_t i = tid; i < n; i += nth) {
        if (SCATTER) __builtin_nontemporal_store(k[i], u + i);
        else k[i] = __builtin_nontemporal_load(u + i);
    }
}

template <bool SCATTER>
__device__ __forceinline__ void move_small(char *user, char *packed, size_t bytes, unsigned unit, unsigned tid,
                                           unsigned nth)
{
    if (bytes == 0) return;
    if (unit == 8) move_units<SCATTER, unsigned long long>(user, packed, bytes, tid, nth);
    else if (unit == 4) move_units<SCATTER, unsigned>(user, packed, bytes, tid, nth);
    else if (unit == 2) move_units<SCATTER, unsigned short>(user, packed, bytes, tid, nth);
    else move_units<SCATTER, unsigned char>(user, packed, bytes, tid, nth);
}

// One piece by `nth` threads (the workgroup, or one wave for a small piece), this one `tid`.
template <bool SCATTER>
__device__ __forceinline__ void move_piece(const GPiece &P, char *packed, unsigned tid, unsigned nth)
{
    char *k = packed + P.poff;
    move_small<SCATTER>(P.user, k, P.head, P.unit, tid, nth);
    if (!P.vec) return;
    FTAR_GLOBAL v4u *U = (FTAR_GLOBAL v4u *)(P.user + P.head), *K = (FTAR_GLOBAL v4u *)(k + P.head);
    size_t i = tid;
    // kUnroll independent 16-byte loads in flight per lane, as the segment kernel's tiles
    for (; i + (size_t)(kUnroll - 1) * nth < P.nvec; i += (size_t)kUnroll * nth) {
        v4u v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++)
            v[u] = SCATTER ? K[i + (size_t)u * nth] : __builtin_nontemporal_load(U + i + (size_t)u * nth);
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            if (SCATTER) __builtin_nontemporal_store(v[u], U + i + (size_t)u * nth);
            else K[i + (size_t)u * nth] = v[u];
        }
    }
    for (; i < P.nvec; i += nth) {
        if (SCATTER) __builtin_nontemporal_store(K[i], U + i);
        else K[i] = __builtin_nontemporal_load(U + i);
    }
    const size_t done = P.head + P.nvec * 16;
    move_small<SCATTER>(P.user + done, k + done, P.bytes - done, P.unit, tid, nth);
}

constexpr size_t kWavePiece = 1024; // a piece below this many bytes is one wave's; the waves take entries in turn

template <bool SCATTER>
__global__ __launch_bounds__(kBlock) void gather_kernel(GatherArgs A)
{
    signal_acquire(A.sig);
    // blockIdx and the wave's number are wave-uniform: readfirstlane keeps the tile bounds, the
    // binary search and the table reads in SGPRs (scalar loads of the table)
    const unsigned b0 = (unsigned)__builtin_amdgcn_readfirstlane((int)blockIdx.x);
    const unsigned nb = (unsigned)__builtin_amdgcn_readfirstlane((int)gridDim.x);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned lane = threadIdx.x & 63;
    // The table is not written while the kernel runs (the copy that filled it is in front of the
    // launch on the stream): read through the constant address space, its uniform loads are
    // scalar loads out of the scalar cache -- the search and the walk are a chain of dependent
    // loads in front of every tile, and as vector loads they cost an L2 round trip each.
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) GEntry *CTab;
#else // (the host pass only parses the kernel)
    typedef const GEntry *CTab;
#endif
    const CTab tab = (CTab)A.tab;
    for (unsigned t = b0; t < A.ntiles; t += nb) {
        const size_t lo = (size_t)t * kTileBytes;
        const size_t hi = lo + kTileBytes < A.total ? lo + kTileBytes : A.total;
        for (int e = __builtin_amdgcn_readfirstlane(gather_first(tab, A.n, lo)); e < A.n; e++) {
            const GEntry E = {tab[e].ptr, tab[e].off, tab[e].bytes};
            GPiece P;
            if (!gather_piece(E, lo, hi, A.packed, A.es, &P)) break; // entries ascend: past the tile
            if (P.bytes >= kWavePiece) move_piece<SCATTER>(P, A.packed, threadIdx.x, kBlock);
            else if ((e & 3) == wave) move_piece<SCATTER>(P, A.packed, lane, 64);
            if (E.off + E.bytes >= hi) break; // the tile ends inside this entry: no look at the next
        }
    }
    signal_done(A.sig);
}

hipError_t launch_gather(const GatherArgs &A, int scatter, unsigned grid, hipStream_t s)
{
    if (!A.packed || !A.tab || A.n < 1 || A.n > kMaxGather || grid == 0 || grid > A.ntiles ||
        (size_t)A.ntiles != (A.total + kTileBytes - 1) / kTileBytes)
        return hipErrorInvalidValue;
    if (scatter) hipLaunchKernelGGL(gather_kernel<true>, dim3(grid), dim3(kBlock), 0, s, A);
    else hipLaunchKernelGGL(gather_kernel<false>, dim3(grid), dim3(kBlock), 0, s, A);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// converting gather / scatter (CPiece, ftar_kernels.h): 2-byte floats <-> packed float32
// ---------------------------------------------------------------------------------
// Widening is exact (bfloat16: the float's upper half; float16: v_cvt_f32_f16 with the f16
// denormal mode on, so subnormals convert, not flush).  Narrowing is ONE rounding to nearest
// even of scale * a, the product one float32 multiplication (subnormals kept: the f32 denormal
// mode is on as well; -ffp-contract=off, and there is nothing beside it to fuse with):
// v_cvt_pk_bf16_f32 as in apply_bf16, v_cvt_f16_f32 / v_cvt_pk_f16_f32 under the default
// rounding mode -- never the cvt_pkrtz builtin, which truncates.
template <typename T> __device__ __forceinline__ float widen16(uint16_t b);
template <> __device__ __forceinline__ float widen16<bf16_t>(uint16_t b) { return bf16_widen(bf16_t{b}); }
template <> __device__ __forceinline__ float widen16<f16_t>(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
// The compiler's own selection for float16 forced one thing: it folds (_Float16)(scale * a) into
// v_fma_mixlo_f16 scale, a, 0 -- an addend of +0 turns a product of -0 into +0, and the
// multiplication is no longer an instruction of its own.  An empty asm statement between the two
// makes the product opaque (it emits nothing), so the multiplication stays v_mul_f32 /
// v_pk_mul_f32 and the conversion v_cvt_f16_f32 / v_cvt_pk_f16_f32.
#define FTAR_OPAQUE_VGPR(x) __asm__("" : "+v"(x))
template <typename T> __device__ __forceinline__ uint16_t narrow1(float a, float scale);
template <> __device__ __forceinline__ uint16_t narrow1<bf16_t>(float a, float scale)
{
    return __builtin_bit_cast(uint16_t, (__bf16)(scale * a));
}
template <> __device__ __forceinline__ uint16_t narrow1<f16_t>(float a, float scale)
{
    float r = scale * a;
    FTAR_OPAQUE_VGPR(r);
    return __builtin_bit_cast(uint16_t, (_Float16)r);
}
template <typename T> __device__ __forceinline__ uint32_t narrow2(f2_t a, float scale);
template <> __device__ __forceinline__ uint32_t narrow2<bf16_t>(f2_t a, float scale)
{
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(a * scale, b2_t));
}
template <> __device__ __forceinline__ uint32_t narrow2<f16_t>(f2_t a, float scale)
{
    f2_t r = a * scale;
    FTAR_OPAQUE_VGPR(r);
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(r, h2_t));
}

// One access of class K: K elements, 2 K bytes of user memory against 4 K bytes of packed memory
// (K = 8: global_load/store_dwordx4 on the user side, two of them on the packed side).
typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v8f __attribute__((ext_vector_type(8)));
template <int K> struct CvtAccess;
template <> struct CvtAccess<8> { typedef v4u U; typedef v8f P; };
template <> struct CvtAccess<4> { typedef v2u U; typedef v4f P; };
template <> struct CvtAccess<2> { typedef unsigned int U; typedef v2f P; };
template <> struct CvtAccess<1> { typedef unsigned short U; typedef float P; };

template <typename T, int K>
__device__ __forceinline__ typename CvtAccess<K>::P widen_group(typename CvtAccess<K>::U u)
{
    uint16_t h[K];
    float f[K];
    __builtin_memcpy(h, &u, 2 * K);
#pragma unroll
    for (int j = 0; j < K; j++) f[j] = widen16<T>(h[j]);
    typename CvtAccess<K>::P p;
    __builtin_memcpy(&p, f, 4 * K);
    return p;
}

template <typename T, int K>
__device__ __forceinline__ typename CvtAccess<K>::U narrow_group(typename CvtAccess<K>::P p, float scale)
{
    typename CvtAccess<K>::U u;
    if constexpr (K == 1) {
        u = narrow1<T>(p, scale);
    } else { // two elements per 32-bit register: one packed multiplication, one packed conversion
        f2_t f[K / 2];
        uint32_t h[K / 2];
        __builtin_memcpy(f, &p, 4 * K);
#pragma unroll
        for (int j = 0; j < K / 2; j++) h[j] = narrow2<T>(f[j], scale);
        __builtin_memcpy(&u, h, 2 * K);
    }
    return u;
}

// `ng` groups of K elements by `nth` threads; user memory non-temporal, packed memory plain (as
// move_units above); kUnroll independent loads in flight per lane, as move_piece
template <typename T, bool SCATTER, int K>
__device__ __forceinline__ void cvt_groups(char *user, char *packed, size_t ng, float scale, unsigned tid, unsigned nth)
{
    typedef typename CvtAccess<K>::U UV;
    typedef typename CvtAccess<K>::P PV;
    FTAR_GLOBAL UV *U = (FTAR_GLOBAL UV *)user;
    FTAR_GLOBAL PV *P = (FTAR_GLOBAL PV *)packed;
    size_t i = tid;
    for (; i + (size_t)(kUnroll - 1) * nth < ng; i += (size_t)kUnroll * nth) {
        if (SCATTER) {
            PV v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) v[u] = P[i + (size_t)u * nth];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) __builtin_nontemporal_store(narrow_group<T, K>(v[u], scale), U + i + (size_t)u * nth);
        } else {
            UV v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) v[u] = __builtin_nontemporal_load(U + i + (size_t)u * nth);
#pragma unroll
            for (int u = 0; u < kUnroll; u++) P[i + (size_t)u * nth] = widen_group<T, K>(v[u]);
        }
    }
    for (; i < ng; i += nth) {
        if (SCATTER) __builtin_nontemporal_store(narrow_group<T, K>(P[i], scale), U + i);
        else P[i] = widen_group<T, K>(__builtin_nontemporal_load(U + i));
    }
}

template <typename T, bool SCATTER>
__device__ __forceinline__ void cvt_move_piece(const CPiece &P, char *packed, float scale, unsigned tid, unsigned nth)
{
    char *k = packed + P.poff;
    cvt_groups<T, SCATTER, 1>(P.user, k, P.head, scale, tid, nth);
    if (P.k == 1) return;
    char *ub = P.user + 2 * P.head, *kb = k + 4 * P.head;
    if (P.k == 8) cvt_groups<T, SCATTER, 8>(ub, kb, P.nvec, scale, tid, nth);
    else if (P.k == 4) cvt_groups<T, SCATTER, 4>(ub, kb, P.nvec, scale, tid, nth);
    else cvt_groups<T, SCATTER, 2>(ub, kb, P.nvec, scale, tid, nth);
    const size_t done = P.head + P.nvec * P.k;
    cvt_groups<T, SCATTER, 1>(P.user + 2 * done, k + 4 * done, P.n - done, scale, tid, nth);
}

// gather_kernel's grid, search and walk (tiles, offsets and kWavePiece in packed bytes)
template <typename T, bool SCATTER>
__global__ __launch_bounds__(kBlock) void gather_cvt_kernel(GatherArgs A, float scale)
{
    signal_acquire(A.sig);
    const unsigned b0 = (unsigned)__builtin_amdgcn_readfirstlane((int)blockIdx.x);
    const unsigned nb = (unsigned)__builtin_amdgcn_readfirstlane((int)gridDim.x);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned lane = threadIdx.x & 63;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) GEntry *CTab; // scalar loads, as gather_kernel's
#else
    typedef const GEntry *CTab;
#endif
    const CTab tab = (CTab)A.tab;
    for (unsigned t = b0; t < A.ntiles; t += nb) {
        const size_t lo = (size_t)t * kTileBytes;
        const size_t hi = lo + kTileBytes < A.total ? lo + kTileBytes : A.total;
        for (int e = __builtin_amdgcn_readfirstlane(gather_first(tab, A.n, lo)); e < A.n; e++) {
            const GEntry E = {tab[e].ptr, tab[e].off, tab[e].bytes};
            CPiece P;
            if (!cvt_piece(E, lo, hi, A.packed, &P)) break;
            const bool big = P.n * 4 >= kWavePiece; // the workgroup's piece, or one wave's
            if (big || (e & 3) == wave) cvt_move_piece<T, SCATTER>(P, A.packed, scale, big ? threadIdx.x : lane, big ? kBlock : 64);
            if (E.off + E.bytes >= hi) break;
        }
    }
    signal_done(A.sig);
}

hipError_t launch_gather_cvt(const GatherArgs &A, int dtype, float scale, int scatter, unsigned grid, hipStream_t s)
{
    if (!A.packed || !A.tab || A.n < 1 || A.n > kMaxGather || grid == 0 || grid > A.ntiles || A.es != 4 || A.total % 4 ||
        (size_t)A.ntiles != (A.total + kTileBytes - 1) / kTileBytes || (dtype != kFloat16 && dtype != kBFloat16))
        return hipErrorInvalidValue;
    if (dtype == kFloat16) {
        if (scatter) hipLaunchKernelGGL((gather_cvt_kernel<f16_t, true>), dim3(grid), dim3(kBlock), 0, s, A, scale);
        else hipLaunchKernelGGL((gather_cvt_kernel<f16_t, false>), dim3(grid), dim3(kBlock), 0, s, A, scale);
    } else {
        if (scatter) hipLaunchKernelGGL((gather_cvt_kernel<bf16_t, true>), dim3(grid), dim3(kBlock), 0, s, A, scale);
        else hipLaunchKernelGGL((gather_cvt_kernel<bf16_t, false>), dim3(grid), dim3(kBlock), 0, s, A, scale);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// mixed gather / scatter: every entry float16, bfloat16 or float32 <-> packed float32
// ---------------------------------------------------------------------------------
// A float32 entry's scatter: user[j] = scale * packed[j], one v_mul_f32 / v_pk_mul_f32 per
// element and nothing beside it (a store follows, so there is no conversion to fold it into: -0
// and subnormal products stay what IEEE says).  GPiece with es = 4: heads, tails and pieces that
// are not congruent mod 16 go word by word (unit = 4 always: user pointers are 4-byte aligned,
// packed offsets multiples of 4), the rest in 16-byte accesses; user side non-temporal, packed
// side plain, kUnroll loads in flight per lane, as move_piece.
__device__ __forceinline__ void scale_words(char *user, char *packed, size_t bytes, float scale, unsigned tid,
                                            unsigned nth)
{
    FTAR_GLOBAL float *u = (FTAR_GLOBAL float *)user, *k = (FTAR_GLOBAL float *)packed;
    const size_t n = bytes / 4;
    for (size_t i = tid; i < n; i += nth) __builtin_nontemporal_store(scale * k[i], u + i);
}

__device__ __forceinline__ void scale_piece(const GPiece &P, char *packed, float scale, unsigned tid, unsigned nth)
{
    char *k = packed + P.poff;
    scale_words(P.user, k, P.head, scale, tid, nth);
    if (!P.vec) return;
    FTAR_GLOBAL v4f *U = (FTAR_GLOBAL v4f *)(P.user + P.head), *K = (FTAR_GLOBAL v4f *)(k + P.head);
    size_t i = tid;
    for (; i + (size_t)(kUnroll - 1) * nth < P.nvec; i += (size_t)kUnroll * nth) {
        v4f v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) v[u] = K[i + (size_t)u * nth];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) __builtin_nontemporal_store(v[u] * scale, U + i + (size_t)u * nth);
    }
    for (; i < P.nvec; i += nth) __builtin_nontemporal_store(K[i] * scale, U + i);
    const size_t done = P.head + P.nvec * 16;
    scale_words(P.user + done, k + done, P.bytes - done, scale, tid, nth);
}

// gather_kernel's grid, search and walk.  The entry's type is one more scalar load (the array
// behind the table, through the constant address space as well) and wave-uniform, so the choice
// of the mover is a uniform branch; the waves of a workgroup may be on small entries of
// different types at the same time.
template <bool SCATTER>
__global__ __launch_bounds__(kBlock) void gather_mix_kernel(GatherArgs A, const unsigned *types, float scale)
{
    signal_acquire(A.sig);
    const unsigned b0 = (unsigned)__builtin_amdgcn_readfirstlane((int)blockIdx.x);
    const unsigned nb = (unsigned)__builtin_amdgcn_readfirstlane((int)gridDim.x);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned lane = threadIdx.x & 63;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) GEntry *CTab; // scalar loads, as gather_kernel's
    typedef const __attribute__((address_space(4))) unsigned *CTy;
#else
    typedef const GEntry *CTab;
    typedef const unsigned *CTy;
#endif
    const CTab tab = (CTab)A.tab;
    const CTy ty = (CTy)types;
    for (unsigned t = b0; t < A.ntiles; t += nb) {
        const size_t lo = (size_t)t * kTileBytes;
        const size_t hi = lo + kTileBytes < A.total ? lo + kTileBytes : A.total;
        for (int e = __builtin_amdgcn_readfirstlane(gather_first(tab, A.n, lo)); e < A.n; e++) {
            const GEntry E = {tab[e].ptr, tab[e].off, tab[e].bytes};
            const size_t pb = E.off > lo ? E.off : lo, pe = E.off + E.bytes < hi ? E.off + E.bytes : hi;
            if (pb >= pe) break;
            const bool big = pe - pb >= kWavePiece; // the workgroup's piece, or one wave's
            if (big || (e & 3) == wave) {
                const unsigned dt = (unsigned)__builtin_amdgcn_readfirstlane((int)ty[e]);
                const unsigned tid = big ? threadIdx.x : lane, nth = big ? kBlock : 64;
                if (dt == (unsigned)kFloat32) {
                    GPiece P;
                    gather_piece(E, lo, hi, A.packed, 4, &P);
                    if (SCATTER) scale_piece(P, A.packed, scale, tid, nth);
                    else move_piece<false>(P, A.packed, tid, nth);
                } else {
                    CPiece P;
                    cvt_piece(E, lo, hi, A.packed, &P);
                    if (dt == (unsigned)kFloat16) cvt_move_piece<f16_t, SCATTER>(P, A.packed, scale, tid, nth);
                    else cvt_move_piece<bf16_t, SCATTER>(P, A.packed, scale, tid, nth);
                }
            }
            if (E.off + E.bytes >= hi) break;
        }
    }
    signal_done(A.sig);
}

hipError_t launch_gather_mix(const GatherArgs &A, const unsigned *types, float scale, int scatter, unsigned grid,
                             hipStream_t s)
{
    if (!A.packed || !A.tab || !types || A.n < 1 || A.n > kMaxGather || grid == 0 || grid > A.ntiles || A.es != 4 ||
        A.total % 4 || (size_t)A.ntiles != (A.total + kTileBytes - 1) / kTileBytes)
        return hipErrorInvalidValue;
    if (scatter) hipLaunchKernelGGL(gather_mix_kernel<true>, dim3(grid), dim3(kBlock), 0, s, A, types, scale);
    else hipLaunchKernelGGL(gather_mix_kernel<false>, dim3(grid), dim3(kBlock), 0, s, A, types, scale);
    return hipGetLastError();
}

hipError_t launch_segments(int dtype, int op, const KSegList &L, unsigned grid, hipStream_t s)
{
    return with_type(dtype, op, [&](auto t) {
        using T = typename decltype(t)::type;
        return with_op<T>(op, [&](auto o) {
            hipLaunchKernelGGL((segment_kernel<T, decltype(o)::value>), dim3(grid), dim3(kBlock), 0, s, L);
            return hipGetLastError();
        });
    });
}

hipError_t launch_reduce_lds(int dtype, int op, void *inout, const void *in, size_t nvec, unsigned grid,
                             hipStream_t s, unsigned nts)
{
    uint4 *io = (uint4 *)inout;
    const uint4 *i = (const uint4 *)in;
    return with_type(dtype, op, [&](auto t) {
        using T = typename decltype(t)::type;
        return with_op<T>(op, [&](auto o) {
            hipLaunchKernelGGL((reduce_lds_kernel<T, decltype(o)::value>), dim3(grid), dim3(kBlock), 0, s, io, i, nvec,
                               nts);
            return hipGetLastError();
        });
    });
}

} // namespace ftar
