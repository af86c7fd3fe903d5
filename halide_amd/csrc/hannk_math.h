// hannk_math.h — the fixed-point helpers of apps/hannk/halide/common_halide.cpp, each restated in the type Halide gives it (DESIGN.md
// §5.12 for the epilogue, §5.13 for the approx_* helpers, §5.14 for the Elementwise interpreter), shared by hannk_conv.hip, hannk_nn.hip and
// hannk_program.hip.  Host and device.
//
// Conventions: a value of a type below 32 bits travels in an int32_t and is wrapped (wrap<BITS>) or saturated (sat<BITS>) wherever
// Halide's type does so; i32 arithmetic wraps through uint32_t.  Shifts: the result has the left operand's type; a negative signed
// count shifts the other way; a count of 32 or more (which Halide leaves to the target) is defined here as shifting everything out.
#pragma once

#include <stdint.h>

namespace hlmi {
namespace hannk_math {

struct Quant {
    int32_t multiplier, shift;
    int32_t zero, lo, hi;   // u8 values
};
// sat_i32((i64(a) * b + 2^30) >> 31): saturates at INT32_MIN * INT32_MIN only
__host__ __device__ inline int32_t multiply_2x_high(int32_t a, int32_t b) {
    const int64_t p = ((int64_t)a * b + ((int64_t)1 << 30)) >> 31;
    return p > 0x7fffffffLL ? 0x7fffffff : (int32_t)p;
}
// run-time signed shift (src/FindIntrinsics.cpp: lower_rounding_shift_right): s < 0 is a wrapping left shift
__host__ __device__ inline int32_t rounding_shift_right(int32_t a, int32_t s) {
    if (s > 0) return (a >> (s & 31)) + ((a >> ((s - 1) & 31)) & 1);
    return (int32_t)((uint32_t)a << ((-s) & 31));
}
__host__ __device__ inline int32_t quantize_i16(int32_t acc, const Quant &q) {
    const int32_t v = rounding_shift_right(multiply_2x_high(acc, q.multiplier), q.shift);
    return v < -32768 ? -32768 : v > 32767 ? 32767 : v;
}
// u8_sat(saturating_add(i16 v, u8 zero)) then Halide's clamp = max(min(v, hi), lo): lo wins where the two cross
__host__ __device__ inline int32_t add_zero_and_relu_u8(int32_t v, int32_t zero, int32_t lo, int32_t hi) {
    v += zero;
    v = v > 32767 ? 32767 : v;                 // saturating_add in int16 (match_types: i16 + u8 is an i16 add)
    v = v < 0 ? 0 : v > 255 ? 255 : v;         // u8_sat
    v = v < hi ? v : hi;
    return v > lo ? v : lo;
}
__host__ __device__ inline int32_t quantize_and_relu_u8(int32_t acc, const Quant &q) {
    return add_zero_and_relu_u8(quantize_i16(acc, q), q.zero, q.lo, q.hi);
}

// ---------------------------------------------------------------------------------------------------------------- types
template<int BITS>
__host__ __device__ inline int32_t wrap(int64_t v) {
    if (BITS == 16) return (int32_t)(int16_t)(uint16_t)(uint64_t)v;
    return (int32_t)(uint32_t)(uint64_t)v;
}
template<int BITS>
__host__ __device__ inline int32_t sat(int64_t v) {
    const int64_t lo = BITS == 16 ? -32768 : -2147483647LL - 1, hi = BITS == 16 ? 32767 : 2147483647LL;
    return (int32_t)(v < lo ? lo : v > hi ? hi : v);
}
// a << c of a signed BITS-bit a with a signed count c
template<int BITS>
__host__ __device__ inline int32_t shl(int32_t a, int32_t c) {
    if (c >= 0) return c >= BITS ? 0 : wrap<BITS>((int64_t)((uint64_t)(int64_t)a << c));
    return c <= -BITS ? (a < 0 ? -1 : 0) : a >> -c;
}
// rounding_mul_shift_right(a, b, BITS - 1), saturating (src/FindIntrinsics.cpp: lower_rounding_mul_shift_right)
template<int BITS>
__host__ __device__ inline int32_t mul2x(int32_t a, int32_t b) {
    if (BITS == 32) return multiply_2x_high(a, b);
    return sat<16>((a * b + (1 << 14)) >> 15);   // |a b| <= 2^30: no overflow
}
__host__ __device__ inline int32_t clz32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int)x);
#else
    return x ? __builtin_clz(x) : 32;
#endif
}

// ---------------------------------------------------------------------------------------------------------------- approx_*
// approx_log2(q, x, q_x, Int(TB)) of an i32 x (common_halide.cpp:71-115); x == 0: clz = 32, floor_log2 = -1
template<int TB>
__host__ __device__ inline int32_t approx_log2(int q, int32_t x, int q_x) {
    const int fl = 31 - clz32((uint32_t)x);                                         // i16
    const int32_t frac1 = wrap<16>(shl<32>(x, 15 - fl)) & 0x7fff;                   // i32 shift, signed count; then i16
    const int32_t frac2 = mul2x<16>(frac1, frac1), frac3 = mul2x<16>(frac2, frac1);
    const int32_t poly = wrap<16>((int64_t)mul2x<16>(2555, frac3) + mul2x<16>(-9421, frac2) + mul2x<16>(23249, frac1) + 5);
    int32_t frac_result;
    if (q < 14) frac_result = (poly >> (14 - q)) + ((poly >> (13 - q)) & 1);        // rounding_shift_right by a positive constant
    else frac_result = shl<TB>(wrap<TB>(poly), q - 14);
    const int32_t floor_result = shl<TB>(wrap<TB>(wrap<16>(fl - q_x)), q);
    return sat<TB>((int64_t)floor_result + frac_result);
}
// approx_exp2(q, x, q_x, Int(TB)) of an XB-bit signed x and a count q_x >= 0 (common_halide.cpp:117-153)
template<int XB, int TB>
__host__ __device__ inline int32_t approx_exp2(int q, int32_t x, uint32_t q_x) {
    const int32_t floor_x = wrap<TB>(q_x >= (uint32_t)XB ? (x < 0 ? -1 : 0) : x >> q_x);
    const int32_t e = sat<TB>(shl<32>(1, wrap<TB>((int64_t)floor_x + q)));          // 1 << (floor_x + q): an i32 shift, saturated to the type
    // i16(x - (floor_x << q_x)): only the residue modulo 2^16 survives the cast, so the width of the inner shift does not matter
    const int32_t d = wrap<16>((int64_t)(uint32_t)x - (q_x >= 32u ? 0u : (uint32_t)floor_x << q_x));
    const int32_t frac1 = shl<16>(d, wrap<16>(15 - (int32_t)wrap<16>(q_x)));
    const int32_t frac2 = mul2x<16>(frac1, frac1), frac3 = mul2x<16>(frac2, frac1);
    int32_t poly = wrap<16>((int64_t)mul2x<16>(2592, frac3) + mul2x<16>(7363, frac2) + mul2x<16>(22812, frac1));
    poly = shl<TB>(poly, TB - 16);
    return sat<TB>((int64_t)e + mul2x<TB>(e, poly));
}
// both evaluate their approx_log2 in the default Int(32) (common_halide.cpp:155-169)
template<int TB>
__host__ __device__ inline int32_t approx_reciprocal(int q, int32_t x) {
    return approx_exp2<32, TB>(q, wrap<32>(-(int64_t)approx_log2<32>(15, x, 0)), 15);
}
template<int TB>
__host__ __device__ inline int32_t approx_reciprocal_sqrt(int q, int32_t x) {
    return approx_exp2<32, TB>(q, wrap<32>(-(int64_t)approx_log2<32>(14, x, 0)), 15);
}

// ---------------------------------------------------------------------------------------------------------------- approx_logistic, approx_tanh
// common_halide.cpp:177-226, as the Elementwise generator instantiates them: x and the result are i16, q_x is a
// run-time signed count of CW bits.  A shift by q_x runs at the wider of its operand's and the count's width (match_bits,
// src/IROperator.cpp:2742-2747): CW = 16 in the generator, where q_x is the i16 expression input2 + arg3; CW = 32 in the reference's own
// test, where it is the i32 Var y.  The constant log_q = 11 reaches approx_exp2 as an i32 immediate in both.
// x >> c of a BITS-bit signed x, signed count
template<int BITS>
__host__ __device__ inline int32_t shr(int32_t a, int32_t c) { return shl<BITS>(a, c == INT32_MIN ? 0x7fffffff : -c); }
// rounding_shift_right(a, s) of an i16 a with a signed i16 count (lower_rounding_shift_right: (a >> s) + (s > 0 & (a >> sat_sub(s, 1))))
__host__ __device__ inline int32_t rounding_shift_right16(int32_t a, int32_t s) {
    if (s <= 0) return shl<16>(a, -s);
    return wrap<16>((int64_t)shr<16>(a, s) + (shr<16>(a, s - 1) & 1));
}
// approx_exp2(16, x, q_x, Int(32)) of an i16 x with a signed count
template<int CW>
__host__ __device__ inline int32_t approx_exp2_q16(int32_t x, int32_t q_x) {
    const int32_t floor_x = shr<CW>(x, q_x);                                          // cast to i32: the value as it is
    const int32_t e = shl<32>(1, wrap<32>((int64_t)floor_x + 16));
    const int32_t d = wrap<16>((int64_t)x - shl<32>(floor_x, q_x));                   // floor_x is an i32: a 32-bit shift whatever CW
    const int32_t frac1 = shl<16>(d, wrap<16>(15 - (int32_t)wrap<16>(q_x)));
    const int32_t frac2 = mul2x<16>(frac1, frac1), frac3 = mul2x<16>(frac2, frac1);
    int32_t poly = wrap<16>((int64_t)mul2x<16>(2592, frac3) + mul2x<16>(7363, frac2) + mul2x<16>(22812, frac1));
    poly = shl<32>(poly, 16);
    return sat<32>((int64_t)e + mul2x<32>(e, poly));
}
// approx_log2_exp2_plus_or_minus_one(q, x, sign, q_x, Int(16)): sign = 1 approx_log2p1_exp2, sign = -1 approx_log2m1_exp2
template<int CW>
__host__ __device__ inline int32_t approx_log2pm1_exp2(int q, int32_t x, int sign, int32_t q_x) {
    const int32_t one_plus = wrap<32>((int64_t)sign * 65536 + approx_exp2_q16<CW>(x, q_x));
    const int32_t raw = approx_log2<16>(q, one_plus, 16);
    const int32_t line = sat<16>(rounding_shift_right(x, wrap<16>((int64_t)wrap<16>(q_x) - q)));   // the widened x: an i32 shift
    return shr<CW>(x, q_x) < 14 ? raw : line;
}
constexpr int LOG2_E_Q14 = 23637;   // lround(1.442695f * 2^14)
template<int CW>
__host__ __device__ inline int32_t approx_logistic(int q, int32_t x, int32_t q_x) {
    const int32_t x2 = mul2x<16>(x, -LOG2_E_Q14);
    const int32_t log2_d = approx_log2pm1_exp2<CW>(11, x2, 1, wrap<CW>((int64_t)q_x - 1));
    return approx_exp2<16, 16>(q, wrap<16>(-(int64_t)log2_d), 11);
}
template<int CW>
__host__ __device__ inline int32_t approx_tanh(int q, int32_t x, int32_t q_x) {
    const int32_t x2 = mul2x<16>(x, LOG2_E_Q14);
    const int32_t ax = wrap<16>(x2 < 0 ? -(int64_t)x2 : x2), c = wrap<CW>((int64_t)q_x - 2);
    const int32_t log2_n = approx_log2pm1_exp2<CW>(11, ax, -1, c), log2_d = approx_log2pm1_exp2<CW>(11, ax, 1, c);
    const int32_t abs_out = approx_exp2<16, 16>(q, wrap<16>((int64_t)log2_n - log2_d), 11);
    return x2 < 0 ? wrap<16>(-(int64_t)abs_out) : x2 == 0 ? 0 : abs_out;
}

// ---------------------------------------------------------------------------------------------------------------- the Elementwise interpreter
// elementwise_generator.cpp:165-177: one instruction on i16 slots; a = slot[arg1], s2 = slot[arg2], arg3 and arg4 the i16 immediates.
// Noop and any code outside 1 .. 10 give 0 (the reference leaves the slot undefined).
constexpr int EW_MAX_INSTRUCTIONS = 20, EW_INPUTS = 5, EW_SLOTS = EW_INPUTS + EW_MAX_INSTRUCTIONS + 1;
__host__ __device__ inline int32_t elementwise_op(int op, int32_t a, int32_t s2, int32_t arg3, int32_t arg4) {
    const int32_t b = wrap<16>((int64_t)s2 + arg3);
    switch (op) {
    case 1: return sat<16>((int64_t)a + b);
    case 2: return sat<16>((int64_t)a - b);
    case 3: return sat<16>((int64_t)mul2x<16>(a, b) + arg4);
    case 4: {
        // i16_sat(rounding_shift_right(widening_mul(a, b), u32(u16(arg4)))): lower_rounding_mul_shift_right's last resort, the only
        // one open to a run-time count (src/FindIntrinsics.cpp:1568-1575)
        const uint32_t s = (uint32_t)arg4 & 0xffffu;
        const int32_t p = a * b;
        return sat<16>(s == 0 ? p : s > 31 ? 0 : (p >> s) + ((p >> (s - 1)) & 1));
    }
    case 5: return rounding_shift_right16(a, b);
    case 6: return a < b ? a : b;
    case 7: return a > b ? a : b;
    case 8: {
        const int32_t v = a < arg4 ? a : arg4;
        return v > arg3 ? v : arg3;
    }
    case 9: return rounding_shift_right16(approx_logistic<16>(15, a, b), wrap<16>(15 - (int64_t)arg4));
    case 10: return rounding_shift_right16(approx_tanh<16>(15, a, b), wrap<16>(15 - (int64_t)arg4));
    default: return 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the ops' element rules
constexpr int ADD_INPUT_SHIFT = 6, ADD_OUTPUT_SHIFT = 16, MUL_INPUT_SHIFT = 6, SOFTMAX_INPUT_SHIFT = 6;   // apps/hannk/halide/constants.h

struct AddParams {
    int32_t zero1, mul1, zero2, mul2, out_zero, lo, hi;
};
__host__ __device__ inline int32_t add_u8(int32_t a, int32_t b, const AddParams &p) {
    const int32_t i1 = shl<16>(a - p.zero1, ADD_INPUT_SHIFT), i2 = shl<16>(b - p.zero2, ADD_INPUT_SHIFT);
    const int32_t s = wrap<32>((int64_t)i1 * p.mul1 + (int64_t)i2 * p.mul2);                    // widening_mul to i32, i32 add
    const int32_t r = sat<16>((s >> ADD_OUTPUT_SHIFT) + ((s >> (ADD_OUTPUT_SHIFT - 1)) & 1));
    return add_zero_and_relu_u8(r, p.out_zero, p.lo, p.hi);
}
struct MulParams {
    int32_t zero1, zero2, out_zero, multiplier;
    uint32_t shift;
    int32_t lo, hi;
};
__host__ __device__ inline int32_t mul_u8(int32_t a, int32_t b, const MulParams &p) {
    const int32_t i1 = shl<16>(a - p.zero1, MUL_INPUT_SHIFT), i2 = shl<16>(b - p.zero2, MUL_INPUT_SHIFT);
    const int32_t m = multiply_2x_high(wrap<32>((int64_t)i1 * i2), p.multiplier);
    // an unsigned count only shifts right
    const int32_t r = p.shift == 0 ? m : p.shift > 31 ? 0 : (m >> p.shift) + ((m >> (p.shift - 1)) & 1);
    return add_zero_and_relu_u8(sat<16>(r), p.out_zero, p.lo, p.hi);
}

struct SoftmaxParams {
    int32_t beta_multiplier;
    uint32_t beta_shift;
    int32_t out_zero, out_multiplier;
    uint32_t out_shift;
};
// exp2_diff(x, y): i16
__host__ __device__ inline int32_t softmax_exp(int32_t v, int32_t row_max, const SoftmaxParams &p) {
    const int32_t diff = shl<16>(v - row_max, SOFTMAX_INPUT_SHIFT);
    return approx_exp2<16, 16>(15, mul2x<16>(diff, p.beta_multiplier), p.beta_shift);
}
__host__ __device__ inline int32_t softmax_inv_sum(int32_t sum) { return approx_reciprocal<16>(30, sum); }
__host__ __device__ inline int32_t softmax_out(int32_t e, int32_t inv, const SoftmaxParams &p) {
    int32_t o = mul2x<16>(mul2x<16>(e, inv), p.out_multiplier);
    const uint32_t s = p.out_shift;
    o = s == 0 ? o : s > 15 ? 0 : (o >> s) + ((o >> (s - 1)) & 1);   // i16, unsigned count
    return add_zero_and_relu_u8(o, p.out_zero, 0, 255);
}
__host__ __device__ inline int32_t l2norm_inv_sqrt(int32_t sum_sq) { return approx_reciprocal_sqrt<32>(15, sum_sq); }
__host__ __device__ inline int32_t l2norm_out(int32_t zeroed, int32_t inv) {
    const int32_t o = wrap<32>((int64_t)zeroed * inv);
    return add_zero_and_relu_u8(sat<16>((o >> 8) + ((o >> 7) & 1)), 128, 0, 255);
}

// average_pool: inv_filter_count = u16_sat(((2 << 16) + n) / (2 n)) with Halide's floor division and x / 0 == 0
__host__ __device__ inline uint32_t pool_inv_count(int32_t n) {
    const int64_t num = (int64_t)wrap<32>((int64_t)131072 + n), den = (int64_t)wrap<32>(2 * (int64_t)n);
    if (den == 0) return 0;
    int64_t q = num / den;
    if ((num % den != 0) && ((num < 0) != (den < 0))) q--;
    return (uint32_t)(q < 0 ? 0 : q > 65535 ? 65535 : q);
}
// clamp(u8_sat(rounding_mul_shift_right(u16 sum, u16 inv, 16)), lo, hi); the u16 result of the multiply cannot exceed 65535
__host__ __device__ inline int32_t pool_average(uint32_t sum16, uint32_t inv, int32_t lo, int32_t hi) {
    uint32_t v = (uint32_t)(((uint64_t)sum16 * inv + 32768u) >> 16);
    v = v > 255 ? 255 : v;
    int32_t r = (int32_t)v < hi ? (int32_t)v : hi;
    return r > lo ? r : lo;
}
// mean: u8((sum + extent / 2) / extent): u32 + i32 is an i32 add (match_types), the division floors, x / 0 == 0, the cast wraps
__host__ __device__ inline int32_t mean_out(uint32_t sum, int32_t extent) {
    if (extent == 0) return 0;
    const int32_t half = extent >> 1;   // floor(extent / 2)
    const int64_t num = (int64_t)wrap<32>((int64_t)(int32_t)sum + half);
    int64_t q = num / extent;
    if ((num % extent != 0) && ((num < 0) != (extent < 0))) q--;
    return (int32_t)(uint8_t)(uint64_t)q;
}

}  // namespace hannk_math
}  // namespace hlmi
