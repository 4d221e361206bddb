// poseidon2_arith.hpp — the signed, bounded-cell arithmetic of the Poseidon2 kernels, usable from host and device.
//
// The same source is compiled into the gfx950 kernels (poseidon2.hip) and into a host checker
// (tests/host_arith_check.cpp, built with g++ by tests/test_host_arith_cpu.py) that drives every helper with extreme and
// random operands, compares against exact 128-bit arithmetic mod P, and asserts the documented bounds and the absence
// of 64-bit overflow (BX_CHECK_BOUNDS).  See the bounds table in poseidon2.hip.
#pragma once
#include "fp.hpp"

#if defined(BX_CHECK_BOUNDS) && !defined(__HIP_DEVICE_COMPILE__)
#include <stdio.h>
#include <stdlib.h>
#define BX_ASSERT_BOUND(cond, what)                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "bound violated: %s (%s:%d)\n", what, __FILE__, __LINE__); \
            abort();                                                             \
        }                                                                        \
    } while (0)
#else
#define BX_ASSERT_BOUND(cond, what) ((void)0)
#endif

// The multiply-add helpers below have two bodies (pinned instructions / plain C, chosen per translation unit by BX_PLAIN_MAD).
// Each flavour lives in its own inline namespace, so the two never share a mangled name: one definition per entity even if the
// build is ever linked with -fgpu-rdc.
#if defined(BX_PLAIN_MAD)
#define BX_MAD_FLAVOUR mad_plain
#else
#define BX_MAD_FLAVOUR mad_pinned
#endif
namespace bx {
inline namespace BX_MAD_FLAVOUR {

constexpr int P2_CELLS = 24;

// ---- representation tracking ------------------------------------------------------------------------------------------
// A cell holds v * c mod P for a per-round constant factor c = R^e (R = 2^32 mod P), not always the Montgomery factor R:
// the external linear layers are homogeneous, so their return to 32 bits can be a bare REDC (factor * R^-1, 2 multiply-class
// instructions) instead of a factor-preserving one (4), and the S-box maps R^e to R^(7e - 6).  With canonical Montgomery
// input (e = 1) the exponents entering the S-boxes of external rounds 0..3 are 0, -7, -56, -399; the layer after round 3
// multiplies by K1_MID = R^2801 to hand the internal rounds (which need one common factor for all cells, i.e. e = 1) the
// standard form back; rounds 4..7 see 1, 0, -7, -56 and the last layer restores e = 1 with K1_END = R^400.  Round
// constants are stored pre-scaled to the representation of the point where they are added (p2_rc_scale).
constexpr uint32_t cx_mul(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)a * b % P); }
constexpr uint32_t cx_pow(uint32_t b, uint64_t e) {
    uint32_t r = 1;
    while (e) {
        if (e & 1) r = cx_mul(r, b);
        b = cx_mul(b, b);
        e >>= 1;
    }
    return r;
}
constexpr uint32_t cx_rpow(int64_t e) { return cx_pow(MONT_ONE, e >= 0 ? (uint64_t)e : (uint64_t)((int64_t)(P - 1) + e)); }
constexpr uint32_t K1_MID = cx_rpow(2801), K2_MID = cx_mul(K1_MID, MONT_ONE);
constexpr uint32_t K1_END = cx_rpow(400), K2_END = cx_mul(K1_END, MONT_ONE);
// factor (power of R) a canonical round constant is multiplied by in the device table; index as in the 213-word layout
// 4x24 external | 21 internal | 4x24 external.  Constants added inside a REDC accumulator carry one extra R.
constexpr uint32_t p2_rc_scale(int i) {
    return i < 24 ? cx_rpow(1) : i < 48 ? cx_rpow(-6) : i < 72 ? cx_rpow(-55) : i < 96 ? cx_rpow(-398)
         : i < 141 ? cx_rpow(2) /* internal rounds and external round 4: added to Montgomery-form cells inside a REDC */
         : i < 165 ? cx_rpow(1) : i < 189 ? cx_rpow(-6) : cx_rpow(-55);
}

// ---- signed Montgomery arithmetic ---------------------------------------------------------------------------------------
// Inside the permutation a cell is a SIGNED 32-bit integer congruent to its value, only bounded in magnitude.  The signed
// reduction  sredc(t) = (t + m*P) / 2^32  with  m = -t * P^-1 mod 2^32 taken in [-2^31, 2^31)  returns
//   r == t * 2^-32 (mod P),   t/2^32 - P/2 <= r < t/2^32 + P/2,
// so a product of two cells of magnitude < P comes back with magnitude < 0.97 P: the set is closed under multiplication
// and NO conditional subtraction is needed anywhere inside the permutation (the unsigned form needed one per S-box plus
// one per reduced cell).  Three instructions per product as before: v_mad_i64_i32, v_mul_lo_u32, v_mad_i64_i32.
// Only the 24 words that leave the permutation are made canonical (v_add + v_min_u32 each).
// Validity: |t| <= SREDC_MAX keeps the result inside an int32 and t + m*P inside an int64.
using i32 = int32_t;
using i64 = int64_t;
constexpr i64 SREDC_MAX = ((i64)0x7fffffff - (i64)(P / 2) - 2) * ((i64)1 << 32);  // = 1.209 P^2

// The multiply-add primitives.  On the device each one is a single pinned instruction: written as plain C, hipcc widens the
// loop-carried cells to i64, forgets that they are sign-extended 32-bit values and emulates 64x64-bit products
// (v_mad_u64_u32 + 2 v_mul_lo + v_add3 per product), or inserts v_ashrrev/v_mov pairs to build sign-extended register
// pairs for its shift-add forms.  The statements are volatile so that the stage-wise source order below (independent chains
// interleaved) survives the scheduler, which otherwise re-serialises each cell's chain to save registers.
// `alt` (mod 4) picks one of four scratch SGPR pairs for the unused carry-out: hipcc separates adjacent inline-asm
// statements whose register operands overlap with an s_nop (an assumed forwarding hazard), and an s_nop after every
// multiply-add costs ~18 % at the kernel's 3 waves per SIMD (profiles/r01_microbench3_mad_forms.jsonl).  Rotating the pair
// and keeping dependent statements a stage apart removes most of them (467 -> 198 in hash_fold); the rest are spread thinly
// enough that removing them is below measurement noise.
// The host versions are the definitions; a translation unit may define BX_PLAIN_MAD to get them on the device too (circuit.hip).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
#define BX_MAD_ASM(op, args, ...)                                                                  \
    do {                                                                                           \
        switch (alt & 3) {                                                                         \
            case 0: asm volatile(op " %0, s[40:41], " args : "=v"(r) : __VA_ARGS__ : "s40", "s41"); break; \
            case 1: asm volatile(op " %0, s[42:43], " args : "=v"(r) : __VA_ARGS__ : "s42", "s43"); break; \
            case 2: asm volatile(op " %0, s[44:45], " args : "=v"(r) : __VA_ARGS__ : "s44", "s45"); break; \
            default: asm volatile(op " %0, s[46:47], " args : "=v"(r) : __VA_ARGS__ : "s46", "s47"); break; \
        }                                                                                          \
    } while (0)
#endif
BX_HD i64 smad(i32 a, i32 b, i64 c, int alt = 0) {  // a*b + c, all signed
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_i64_i32", "%1, %2, %3", "v"(a), "v"(b), "v"(c));
    return r;
#else
    (void)alt;
    return (i64)a * (i64)b + c;
#endif
}
BX_HD i64 smul(i32 a, i32 b, int alt = 0) {  // a*b
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_i64_i32", "%1, %2, 0", "v"(a), "v"(b));
    return r;
#else
    (void)alt;
    return (i64)a * (i64)b;
#endif
}
BX_HD i64 smad_c64(i32 a, i32 b, i64 c, int alt = 0) {  // a*b + c, c a wave-uniform 64-bit constant: an SGPR pair, one constant-bus read
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_i64_i32", "%1, %2, %3", "v"(a), "v"(b), "s"(c));
    return r;
#else
    (void)alt;
    return (i64)a * (i64)b + c;
#endif
}
BX_HD i64 smad_k(i32 a, uint32_t k, i64 c, int alt = 0) {  // a*k + c, k a wave-uniform constant < 2^31 (scalar operand)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_i64_i32", "%1, %2, %3", "v"(a), "s"(k), "v"(c));
    return r;
#else
    (void)alt;
    return (i64)a * (i64)k + c;
#endif
}
BX_HD i64 smul_k(i32 a, uint32_t k, int alt = 0) {  // a*k
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_i64_i32", "%1, %2, 0", "v"(a), "s"(k));
    return r;
#else
    (void)alt;
    return (i64)a * (i64)k;
#endif
}
BX_HD i64 smad_s(i32 a, i32 k, i64 c, int alt = 0) {  // a*k + c, k a SIGNED wave-uniform constant (scalar operand): centred constants
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_i64_i32", "%1, %2, %3", "v"(a), "s"(k), "v"(c));
    return r;
#else
    (void)alt;
    return (i64)a * (i64)k + c;
#endif
}
BX_HD i64 smul_s(i32 a, i32 k, int alt = 0) {  // a*k, k signed and wave-uniform
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_i64_i32", "%1, %2, 0", "v"(a), "s"(k));
    return r;
#else
    (void)alt;
    return (i64)a * (i64)k;
#endif
}
template <int K>
BX_HD i64 smadc(i32 a, i64 c, int alt = 0) {  // a*K + c, K an inline constant
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_i64_i32", "%1, %3, %2", "v"(a), "v"(c), "n"(K));
    return r;
#else
    (void)alt;
    return (i64)a * K + c;
#endif
}
template <int K>
BX_HD i64 smulc(i32 a, int alt = 0) {  // a*K
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_i64_i32", "%1, %2, 0", "v"(a), "n"(K));
    return r;
#else
    (void)alt;
    return (i64)a * K;
#endif
}
BX_HD i64 add_u32(i64 c, uint32_t k, int alt = 0) {  // c + k, k an unsigned wave-uniform word (round constant)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_u64_u32", "%1, 1, %2", "s"(k), "v"(c));
    return r;
#else
    (void)alt;
    return c + (i64)k;
#endif
}
BX_HD i64 umul_k(uint32_t a, uint32_t k, int alt = 0) {  // a*k, both unsigned
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i64 r;
    BX_MAD_ASM("v_mad_u64_u32", "%1, %2, 0", "v"(a), "s"(k));
    return r;
#else
    (void)alt;
    return (i64)((uint64_t)a * (uint64_t)k);
#endif
}
BX_HD i32 mont_m(i64 t) {  // m = -t * P^-1 mod 2^32 as a signed word (pinned so that a stage's 24 low products stay together)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BX_PLAIN_MAD)
    i32 m;
    asm volatile("v_mul_lo_u32 %0, %1, %2" : "=v"(m) : "v"((uint32_t)t), "s"(NEG_P_INV));
    return m;
#else
    return (i32)((uint32_t)t * NEG_P_INV);
#endif
}
BX_HD i32 sredc(i64 t, int alt = 0) {
    BX_ASSERT_BOUND(t <= SREDC_MAX && t >= -SREDC_MAX, "sredc operand");
    const i32 m = mont_m(t);
    return (i32)(smad_k(m, P, t, alt) >> 32);  // exact: the low word of the sum is zero
}
BX_HD i64 iabs64(i64 v) { return v < 0 ? -v : v; }

// magnitude bounds (integers); ub(T) = T/2^32 + P/2 + 1 is the magnitude bound of sredc(t) for |t| <= T
constexpr i64 ub(i64 T) { return (T >> 32) + (i64)(P / 2) + 1; }
constexpr i64 B_IN = (i64)P - 1;                      // cells entering the permutation (canonical)
constexpr i64 B_Y = 112 * ((i64)1 << 31);             // any external-layer output: 112 * max cell magnitude (< 2^31)
constexpr i64 B_EXT = ub(B_Y + (i64)P);               // redc64s output = S-box input of the external rounds: P/2 + 58
constexpr i64 B_MIDOUT = ub(((i64)1 << 32) * K1_MID + ((B_Y >> 32) + 1) * (i64)K2_MID + 2 * (i64)P);  // cells entering the internal rounds
constexpr i64 B_SUMR = ub(((i64)1 << 31) * R2 + 33 * (i64)R3);  // sum_r: balanced low word times R2 (0.791 P)
// internal-round cells: B -> ub(P * B + B_SUMR + P) has its fixed point at 0.9412 P; 0.945 P is an invariant upper bound
constexpr i64 B_INT = (i64)((double)P * 0.945);
static_assert(ub((i64)(P - 1) * B_INT + B_SUMR + (i64)P) <= B_INT && B_MIDOUT <= B_INT, "internal-round bound is not invariant");
static_assert((i64)(P - 1) * B_INT + B_SUMR + (i64)P <= SREDC_MAX && B_INT * B_INT <= SREDC_MAX, "internal-round products overflow sredc");
static_assert(24 * B_INT < ((i64)1 << 37), "internal sum");

BX_HD uint64_t mad64(uint32_t a, uint32_t b, uint64_t c) { return (uint64_t)a * (uint64_t)b + c; }

// N independent reductions, issued stage by stage (all low products, then all corrections): the pinned primitives are
// opaque to the compiler's scheduler, so independent chains are interleaved here, in the source, to keep dependent
// multiply-adds of one cell apart.
template <int N>
BX_HD void sredc_n(const i64* t, i32* r) {
    i32 m[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        BX_ASSERT_BOUND(t[i] <= SREDC_MAX && t[i] >= -SREDC_MAX, "sredc operand");
        m[i] = mont_m(t[i]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = (i32)(smad_k(m[i], P, t[i], i & 3) >> 32);
}

// x^7 * 2^(-6*32) for |x| <= B_INT: four signed products, no subtraction.  |x2| < 0.92 P, |x3|, |x4| < 0.91 P, |x7| < 0.88 P.
BX_HD i32 sbox7s(i32 x) {
    BX_ASSERT_BOUND(iabs64(x) <= B_INT, "sbox input");
    const i32 x2 = sredc(smul(x, x));
    const i32 x3 = sredc(smul(x2, x));
    const i32 x4 = sredc(smul(x2, x2));
    return sredc(smul(x3, x4));
}
// The S-box that also adds the NEXT external round's constants.  The external layer is linear, M x + rc = M (x + c) with c = M^-1 rc,
// and the last product of an S-box is a multiply-add whose addend is otherwise the literal 0: with K = c * 2^32 mod P (canonical) in
// that addend, sredc(x3 x4 + K) == x^7 + c, and the reduction behind the layer is a bare sredc with no constant (sredc_all) instead of
// a 64-bit add per cell (redc64s_all).  K is wave-uniform and comes as a 64-bit scalar operand (smad_c64); p2_fold_consts derives it.
// |x3 x4 + K| <= 0.907 * 0.896 P^2 + P, and the output bound of the S-box grows by at most 1.
constexpr i64 B_X2 = ub(B_INT * B_INT), B_X3 = ub(B_X2 * B_INT), B_X4 = ub(B_X2 * B_X2);
constexpr i64 T_SBOX_K = B_X3 * B_X4 + (i64)P - 1;  // the last product plus a folded constant
constexpr i64 B_SBOX_K = ub(T_SBOX_K);               // ... reduced: the cells entering an external layer
static_assert(T_SBOX_K <= SREDC_MAX && B_SBOX_K <= ub(B_X3 * B_X4) + 1 && B_SBOX_K <= B_INT, "S-box with a folded constant leaves its bounds");
// the S-box on N cells at once, stage-wise; HAS_K: K[i] rides on the last product of cell i
template <int N, bool HAS_K>
BX_HD void sbox7s_stages(i32* x, const i64* K) {
    i64 t[N], u[N];
    i32 x2[N], x3[N], x4[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        BX_ASSERT_BOUND(iabs64(x[i]) <= B_INT, "sbox input");
        t[i] = smul(x[i], x[i], i & 3);
    }
    sredc_n<N>(t, x2);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        t[i] = smul(x2[i], x[i], 2 * i);
        u[i] = smul(x2[i], x2[i], 2 * i + 1);
    }
    sredc_n<N>(t, x3);
    sredc_n<N>(u, x4);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if constexpr (HAS_K) {
            BX_ASSERT_BOUND(K[i] >= 0 && K[i] < (i64)P, "folded round constant");
            t[i] = smad_c64(x3[i], x4[i], K[i], i & 3);
            BX_ASSERT_BOUND(iabs64(t[i]) <= T_SBOX_K, "sbox last product");
        } else {
            t[i] = smul(x3[i], x4[i], i & 3);
        }
    }
    sredc_n<N>(t, x);
    if constexpr (HAS_K) {
#pragma unroll
        for (int i = 0; i < N; ++i) BX_ASSERT_BOUND(iabs64(x[i]) <= B_SBOX_K, "sbox output");
    }
}
template <int N>
BX_HD void sbox7s_n(i32* x) { sbox7s_stages<N, false>(x, nullptr); }
template <int N>
BX_HD void sbox7s_n(i32* x, const i64* K) { sbox7s_stages<N, true>(x, K); }

// Bare REDC of an external-layer output plus a pre-scaled round constant (canonical, < P):  r == (y + rc) * 2^-32 (mod P),
// |r| <= B_EXT.  3 instructions (64-bit add, v_mul_lo, v_mad_i64_i32).
BX_HD i32 redc64s(i64 y, uint32_t rc) {
    BX_ASSERT_BOUND(iabs64(y) <= B_Y, "external layer output");
    const i32 r = sredc(add_u32(y, rc));
    BX_ASSERT_BOUND(iabs64(r) <= B_EXT, "redc64s output");
    return r;
}

// the 24 bare reductions of a layer, stage-wise; rc = 24 pre-scaled constants
BX_HD void redc64s_all(const i64* y, const uint32_t* rc, i32* s) {
    constexpr int H = P2_CELLS / 2;  // two halves: 12 chains are enough ILP and halve the live temporaries
#pragma unroll
    for (int h = 0; h < P2_CELLS; h += H) {
        i64 acc[H];
#pragma unroll
        for (int i = 0; i < H; ++i) {
            BX_ASSERT_BOUND(iabs64(y[h + i]) <= B_Y, "external layer output");
            acc[i] = add_u32(y[h + i], rc[h + i], i & 3);
        }
        sredc_n<H>(acc, s + h);
    }
#pragma unroll
    for (int i = 0; i < P2_CELLS; ++i) BX_ASSERT_BOUND(iabs64(s[i]) <= B_EXT, "redc64s output");
}

// the 24 bare reductions of a layer whose round constants came in with the S-boxes in front of it (sbox7s_n with K): r == y * 2^-32
// (mod P), |r| <= B_EXT, 2 instructions per cell; the same two halves
BX_HD void sredc_all(const i64* y, i32* s) {
    constexpr int H = P2_CELLS / 2;
#pragma unroll
    for (int i = 0; i < P2_CELLS; ++i) BX_ASSERT_BOUND(iabs64(y[i]) <= B_Y, "external layer output");
#pragma unroll
    for (int h = 0; h < P2_CELLS; h += H) sredc_n<H>(y + h, s + h);
#pragma unroll
    for (int i = 0; i < P2_CELLS; ++i) BX_ASSERT_BOUND(iabs64(s[i]) <= B_EXT, "sredc_all output");
}

// REDC with a change of representation:  r == (y * K1 + add) * 2^-32 (mod P),  K2 = K1 * 2^32 mod P,  y = y_hi * 2^32 + y_lo
// with y_lo unsigned, y_hi signed:  acc = y_lo*K1 + y_hi*K2 + add  in (-(|y_hi|)*P, 2^32 * K1 + ...),  |r| < K1 + P/2 + 60.
template <uint32_t K1, uint32_t K2, bool HAS_ADD = true>
BX_HD i32 red64ks(i64 y, uint32_t add) {
    BX_ASSERT_BOUND(iabs64(y) <= B_Y, "external layer output");
    static_assert(K1 < (1u << 29) && K2 < P, "correction constant too large for the accumulator bound");
    i64 acc = umul_k((uint32_t)y, K1);
    if (HAS_ADD) acc = add_u32(acc, add);
    return sredc(smad_k((i32)(y >> 32), K2, acc));
}
// the representation-changing reductions of a layer's cells [LO, HI) (default: all 24), stage-wise, at most 12 chains at a time;
// only cell 0 may carry an addend.  Cells outside the range are neither read nor written.
template <uint32_t K1, uint32_t K2, bool HAS_ADD0, int LO = 0, int HI = P2_CELLS>
BX_HD void red64ks_all(const i64* y, uint32_t add0, i32* s) {
    static_assert(K1 < (1u << 29) && K2 < P, "correction constant too large for the accumulator bound");
    static_assert(0 <= LO && LO < HI && HI <= P2_CELLS && (!HAS_ADD0 || LO == 0), "live range");
    constexpr int H = HI - LO < P2_CELLS / 2 ? HI - LO : P2_CELLS / 2;
    static_assert((HI - LO) % H == 0, "live range: a whole number of stages");
#pragma unroll
    for (int h = LO; h < HI; h += H) {
        i64 acc[H];
#pragma unroll
        for (int i = 0; i < H; ++i) {
            BX_ASSERT_BOUND(iabs64(y[h + i]) <= B_Y, "external layer output");
            acc[i] = umul_k((uint32_t)y[h + i], K1, i & 3);
        }
        if (HAS_ADD0 && h == 0) acc[0] = add_u32(acc[0], add0, 0);
#pragma unroll
        for (int i = 0; i < H; ++i) acc[i] = smad_k((i32)(y[h + i] >> 32), K2, acc[i], (i + 1) & 3);
        sredc_n<H>(acc, s + h);
    }
}

// external layer circ(2*M4, M4, ..., M4) on signed cells, unreduced 64-bit outputs:
//   w_k = M4 * x_k,  T = sum_k w_k,  y_k = w_k + T.   M4 by the Poseidon2 addition chain (appendix B):
//   t0 = a+b, t1 = c+d, t2 = 2b + t1, t3 = 2d + t0, t4 = 4 t1 + t3, t5 = 4 t0 + t2, w = [t3+t5, t5, t2+t4, t4].
// Rows of the whole layer sum to <= 112, so |y| <= 112 * 2^31 = B_Y for any int32 cells.
// Two parts: m_ext64s_core leaves the blocks w_k in y and the column sums T in t (every output needs all of it), and
// m_ext64s_finish<LO, HI> adds T to the cells [LO, HI) only: the last layer of a permutation whose caller reads 8 cells finishes
// 8 (poseidon2_mix<LO, HI>), and the pinned reductions behind it run on those 8.
BX_HD void m_ext64s_core(const i32* s, i64* y, i64* t) {
    // The 4-cell groups advance three at a time (see sredc_n): enough independent chains to keep dependent multiply-adds
    // apart, and half the live 64-bit temporaries of advancing all six together (131 -> <= 128 VGPRs = a fourth wave per SIMD).
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        i64 t0[3], t1[3], t2[3], t3[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int g = 3 * h + q;
            t0[q] = smulc<1>(s[4 * g], 2 * q);
            t1[q] = smulc<1>(s[4 * g + 2], 2 * q + 1);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int g = 3 * h + q;
            t0[q] = smadc<1>(s[4 * g + 1], t0[q], 2 * q + 2);
            t1[q] = smadc<1>(s[4 * g + 3], t1[q], 2 * q + 3);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int g = 3 * h + q;
            t2[q] = smadc<2>(s[4 * g + 1], t1[q], 2 * q);
            t3[q] = smadc<2>(s[4 * g + 3], t0[q], 2 * q + 1);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int g = 3 * h + q;
            const i64 t4 = t1[q] * 4 + t3[q], t5 = t0[q] * 4 + t2[q];
            y[4 * g] = t3[q] + t5;
            y[4 * g + 1] = t5;
            y[4 * g + 2] = t2[q] + t4;
            y[4 * g + 3] = t4;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t[j] = y[j];
#pragma unroll
        for (int k = 4; k < P2_CELLS; k += 4) t[j] += y[k + j];
    }
}
template <int LO = 0, int HI = P2_CELLS>
BX_HD void m_ext64s_finish(i64* y, const i64* t) {
    static_assert(0 <= LO && LO < HI && HI <= P2_CELLS, "live range");
#pragma unroll
    for (int i = LO; i < HI; ++i) y[i] += t[i & 3];
}
BX_HD void m_ext64s(const i32* s, i64* y) {
    i64 t[4];
    m_ext64s_core(s, y, t);
    m_ext64s_finish(y, t);
}

// internal rounds: sum of the 24 cells (|sum| < 2^37) -> sum * 2^32 mod P with |result| <= B_SUMR.  The low word is taken
// BALANCED (in [-2^31, 2^31)) so that its product with R2 stays within +-2^31 R2 and the result within 0.791 P.
BX_HD i32 internal_sum_rs(i64 sum) {
    BX_ASSERT_BOUND(iabs64(sum) < ((i64)1 << 37), "internal sum < 2^37");
    const i32 lo = (i32)(uint32_t)sum;
    const i32 hi = (i32)(sum >> 32) - (lo >> 31);  // sum = hi * 2^32 + lo with lo signed
    const i32 r = sredc(smad_k(hi, R3, smul_k(lo, R2)));
    BX_ASSERT_BOUND(iabs64(r) <= B_SUMR, "sum_r");
    return r;
}
// one internal round on all cells: s[0] <- S-box, sum, s[i] <- sredc(diag[i] * s[i] + sum_r [+ rc]).
// RC_ALL = false: only cell 0 gets the constant rc[0]; true: every cell i gets rc[i] (the last internal round).
template <bool RC_ALL>
BX_HD void internal_round(i32* s, const uint32_t* diag, const uint32_t* rc) {
    // The S-box of cell 0 is one dependent chain of 12 instructions; the sum of the other 23 cells does not depend on it and
    // is issued in between (two partial sums), so that no two adjacent statements depend on each other.  The trailing
    // argument of each primitive is its position in the instruction stream (carry-out pair rotation).
    BX_ASSERT_BOUND(iabs64(s[0]) <= B_INT, "sbox input");
    i64 pa = smulc<1>(s[1], 0), pb = smulc<1>(s[2], 1);
    i64 t = smul(s[0], s[0], 2);                                    // x^2
    pa = smadc<1>(s[3], pa, 3);
    i32 m = mont_m(t);
    pb = smadc<1>(s[4], pb, 0);
    const i32 x2 = (i32)(smad_k(m, P, t, 1) >> 32);
    pa = smadc<1>(s[5], pa, 2);
    t = smul(x2, s[0], 3);                                          // x^3
    pb = smadc<1>(s[6], pb, 0);
    i64 u = smul(x2, x2, 1);                                        // x^4
    pa = smadc<1>(s[7], pa, 2);
    m = mont_m(t);
    pb = smadc<1>(s[8], pb, 3);
    i32 m2 = mont_m(u);
    pa = smadc<1>(s[9], pa, 0);
    const i32 x3 = (i32)(smad_k(m, P, t, 1) >> 32);
    pb = smadc<1>(s[10], pb, 2);
    const i32 x4 = (i32)(smad_k(m2, P, u, 3) >> 32);
    pa = smadc<1>(s[11], pa, 0);
    t = smul(x3, x4, 1);                                            // x^7
    pb = smadc<1>(s[12], pb, 2);
    pa = smadc<1>(s[13], pa, 3);
    m = mont_m(t);
    pb = smadc<1>(s[14], pb, 0);
    pa = smadc<1>(s[15], pa, 1);
    s[0] = (i32)(smad_k(m, P, t, 2) >> 32);
#pragma unroll
    for (int i = 16; i < P2_CELLS; ++i) {
        if (i & 1) pa = smadc<1>(s[i], pa, i + 3);
        else pb = smadc<1>(s[i], pb, i + 3);
    }
    pa = smadc<1>(s[0], pa, 3);
    const i64 sum = pa + pb;
    const i64 c = smulc<1>(internal_sum_rs(sum), 1);
    constexpr int H = P2_CELLS / 2;
#pragma unroll
    for (int h = 0; h < P2_CELLS; h += H) {
        i64 tt[H];
#pragma unroll
        for (int i = 0; i < H; ++i) {
            if (RC_ALL || h + i == 0)
                tt[i] = smad_k(s[h + i], diag[h + i], add_u32(c, rc[h + i], 2 * i + 2), 2 * i + 3);  // diag < P < 2^31: a scalar operand
            else
                tt[i] = smad_k(s[h + i], diag[h + i], c, i + 2);
        }
        sredc_n<H>(tt, s + h);
    }
#pragma unroll
    for (int i = 0; i < P2_CELLS; ++i) BX_ASSERT_BOUND(iabs64(s[i]) <= B_INT, "internal cell");
}

// canonical word -> the representative in [-P/2, P/2] (pool entries of cons_sum, the weights and operands of lazy_ext.hpp)
BX_HD i32 fp_centre(uint32_t v) { return (i32)v - (v > P / 2 ? (i32)P : 0); }

// ---- two internal rounds in one step ------------------------------------------------------------------------------------
// Cells 1..23 are linear in the internal rounds: with v the cell values, d the diagonal and V1, V2 the sums of rounds A and B,
// two rounds give  z_i = d_i^2 v_i + d_i V1 + V2  (i >= 1), so those cells return to 32 bits once per TWO rounds: two
// multiply-adds and one reduction per cell instead of two of each.  Cell 0 (the S-box) is materialised in every round as before.
// Per-cell constants, CENTRED to [-P/2, P/2] (scalar operands like diag[]; p2_pair_consts derives them from the diagonal):
//   E_i = d_i^2 R,  A_i = d_i R^2  (i >= 1);  E_0 = the centred diagonal word of cell 0 (its multiplier in both rounds), A_0 unused.
// With x the cells before round A (x_i == v_i R), x0' = sbox(x0):
//   sum1 = x0' + sum_{i>=1} x_i  (64 bits)        sig1 = sredc(fold64(sum1))                   == V1
//   y0 = sredc(E_0 x0' + sig1 R2 + rcA)           y0' = sbox(y0)
//   t2 = sum_{i>=1} A_i x_i + sig1 (23 R3) + y0' R2                                             == V2 R^3
//   sig2 = sredc(t2) == V2 R^2                    z0 = sredc(E_0 y0' + sig2 + rcB)
//   z_i = sredc(E_i x_i + A_i sig1 + sig2)
// The dot product does not depend on the S-boxes and is issued between their instructions, as two chains of groups of four
// products.  A group (< 2^63) is FOLDED, g -> hi(g) R + lo(g) (congruent, < 0.14 P^2), and the next group accumulates on top
// of the folded value; the last group takes both chains, three products and the late term y0' R2.
// Every magnitude below is a static_assert; the host build asserts them per value (BX_CHECK_BOUNDS, tests/p2_paired_check.cpp).
constexpr i64 fold_ub(i64 T) { return ((T >> 32) + 1) * (i64)MONT_ONE + ((i64)1 << 32); }  // |fold64(g)| for |g| <= T
constexpr i64 B_K = (i64)(P / 2);                                                                // centred constants
constexpr i64 B_SBOX = ub(ub(ub(B_INT * B_INT) * B_INT) * ub(ub(B_INT * B_INT) * ub(B_INT * B_INT)));  // sbox7s output: 0.881 P
constexpr i64 B_SIG1 = ub(fold_ub((i64)1 << 37));                                                // P/2 + 4
constexpr i64 T_DOT = 4 * B_K * B_INT + B_K * B_SIG1;  // a group: four products and (first group) the sig1 term, or a folded group below four products
static_assert(T_DOT <= INT64_MAX && fold_ub(T_DOT) + 4 * B_K * B_INT <= T_DOT, "dot-product group overflows 64 bits");
constexpr i64 T_LAST = 2 * fold_ub(T_DOT) + 3 * B_K * B_INT + B_SBOX * (i64)R2;  // both chains, three products, the late term
static_assert(T_LAST <= INT64_MAX && fold_ub(T_LAST) <= SREDC_MAX, "last dot-product group overflows");
constexpr i64 B_SIG2 = ub(fold_ub(T_LAST));                                                      // 0.563 P
constexpr i64 T_PAIR0 = B_K * B_SBOX + B_SIG1 * (i64)R2 + (i64)P;                                // cell 0, either round
constexpr i64 T_PAIRI = B_K * B_INT + B_K * B_SIG1 + B_SIG2;                                     // cells 1..23
static_assert(B_SIG2 <= B_SIG1 * (i64)R2 && T_PAIR0 <= SREDC_MAX && ub(T_PAIR0) <= B_INT, "paired rounds: cell 0 leaves the internal-round bound");
static_assert(T_PAIRI <= SREDC_MAX && ub(T_PAIRI) <= B_INT, "paired rounds: cells 1..23 leave the internal-round bound");
constexpr i32 K23R3 = (i32)cx_mul(23u, R3) - (cx_mul(23u, R3) > P / 2 ? (i32)P : 0);             // 23 R^3, centred

// g -> hi(g) * R + lo(g) with lo unsigned: congruent to g mod P, one multiply-add
// On the device each fold is preceded by one v_mov_b32 (seven per paired step): the multiply-add takes its addend only as a 64-bit
// register pair, so the zero-extended low word {lo, 0} has to be built beside a register that holds zero.  The move is needed:
// adding the pair of g itself would need the multiplier R - 2^32 = -2P, which is not a 32-bit word, and adding lo through a
// second multiply-add (lo * 1 + hi * R) replaces a 2-cycle move by a 4-cycle multiply-class instruction.
BX_HD i64 fold64(i64 g, int alt = 0) { return smad_k((i32)(g >> 32), MONT_ONE, (i64)(uint32_t)g, alt); }
// the constants of the paired rounds from the Montgomery diagonal: E[24] then A[24]
BX_HD void p2_pair_consts(const uint32_t* diag, i32* E, i32* A) {
    E[0] = fp_centre(diag[0]);
    A[0] = 0;
    for (int i = 1; i < P2_CELLS; ++i) {
        E[i] = fp_centre(fp_mul(diag[i], diag[i]));
        A[i] = fp_centre(fp_mul(diag[i], R2));
    }
}
// rounds A and B on all cells; rc[0], rc[1]: their constants (cell 0), scaled like internal_round's
BX_HD void internal_round_pair(i32* s, const i32* E, const i32* A, const uint32_t* rc) {
    // Stage-wise like internal_round: the two S-box chains are dependent instruction by instruction, and the sum, the dot product
    // and its folds are issued in between.  The trailing argument is the carry-out pair rotation.
    BX_ASSERT_BOUND(iabs64(s[0]) <= B_INT, "sbox input");
    i64 pa = smulc<1>(s[1], 0), pb = smulc<1>(s[2], 1);
    i64 t = smul(s[0], s[0], 2);                                    // x^2
    pa = smadc<1>(s[3], pa, 3);
    i32 m = mont_m(t);
    pb = smadc<1>(s[4], pb, 0);
    i32 x2 = (i32)(smad_k(m, P, t, 1) >> 32);
    pa = smadc<1>(s[5], pa, 2);
    t = smul(x2, s[0], 3);                                          // x^3
    pb = smadc<1>(s[6], pb, 0);
    i64 u = smul(x2, x2, 1);                                        // x^4
    pa = smadc<1>(s[7], pa, 2);
    m = mont_m(t);
    pb = smadc<1>(s[8], pb, 3);
    i32 m2 = mont_m(u);
    pa = smadc<1>(s[9], pa, 0);
    i32 x3 = (i32)(smad_k(m, P, t, 1) >> 32);
    pb = smadc<1>(s[10], pb, 2);
    i32 x4 = (i32)(smad_k(m2, P, u, 3) >> 32);
    pa = smadc<1>(s[11], pa, 0);
    t = smul(x3, x4, 1);                                            // x^7
    pb = smadc<1>(s[12], pb, 2);
    pa = smadc<1>(s[13], pa, 3);
    m = mont_m(t);
    pb = smadc<1>(s[14], pb, 0);
    pa = smadc<1>(s[15], pa, 1);
    const i32 x0 = (i32)(smad_k(m, P, t, 2) >> 32);                 // round A's S-box output
#pragma unroll
    for (int i = 16; i < P2_CELLS; ++i) {
        if (i & 1) pa = smadc<1>(s[i], pa, i + 3);
        else pb = smadc<1>(s[i], pb, i + 3);
    }
    pa = smadc<1>(x0, pa, 3);
    i64 gx = smul_s(s[1], A[1], 0), gy = smul_s(s[5], A[5], 1);     // the two chains of the dot product
    const i64 sum1 = pa + pb;
    BX_ASSERT_BOUND(iabs64(sum1) < ((i64)1 << 37) && iabs64(x0) <= B_SBOX, "internal sum < 2^37");
    i64 a0 = smul_s(x0, E[0], 2);
    i64 f = fold64(sum1, 3);
    gx = smad_s(s[2], A[2], gx, 0);
    m = mont_m(f);
    gy = smad_s(s[6], A[6], gy, 1);
    const i32 sig1 = (i32)(smad_k(m, P, f, 2) >> 32);
    BX_ASSERT_BOUND(iabs64(sig1) <= B_SIG1, "sig1");
    gx = smad_s(s[3], A[3], gx, 3);
    gy = smad_s(s[7], A[7], gy, 0);
    a0 = smad_k(sig1, R2, a0, 1);
    gx = smad_s(s[4], A[4], gx, 2);
    a0 = add_u32(a0, rc[0], 3);
    BX_ASSERT_BOUND(iabs64(a0) <= T_PAIR0, "cell 0, round A");
    gy = smad_s(s[8], A[8], gy, 0);
    m = mont_m(a0);
    gx = smad_s(sig1, K23R3, gx, 1);
    const i32 y0 = (i32)(smad_k(m, P, a0, 2) >> 32);
    BX_ASSERT_BOUND(iabs64(y0) <= B_INT && iabs64(gx) <= T_DOT && iabs64(gy) <= T_DOT, "sbox input");
    i64 fx = fold64(gx, 3);
    t = smul(y0, y0, 0);                                            // round B's S-box
    i64 fy = fold64(gy, 1);
    gx = smad_s(s[9], A[9], fx, 2);
    m = mont_m(t);
    gy = smad_s(s[13], A[13], fy, 3);
    x2 = (i32)(smad_k(m, P, t, 0) >> 32);
    gx = smad_s(s[10], A[10], gx, 1);
    gy = smad_s(s[14], A[14], gy, 2);
    t = smul(x2, y0, 3);
    gx = smad_s(s[11], A[11], gx, 0);
    u = smul(x2, x2, 1);
    gy = smad_s(s[15], A[15], gy, 2);
    m = mont_m(t);
    gx = smad_s(s[12], A[12], gx, 3);
    m2 = mont_m(u);
    gy = smad_s(s[16], A[16], gy, 0);
    x3 = (i32)(smad_k(m, P, t, 1) >> 32);
    BX_ASSERT_BOUND(iabs64(gx) <= T_DOT && iabs64(gy) <= T_DOT, "dot-product group");
    fx = fold64(gx, 2);
    x4 = (i32)(smad_k(m2, P, u, 3) >> 32);
    fy = fold64(gy, 0);
    t = smul(x3, x4, 1);
    gx = smad_s(s[17], A[17], fx, 2);
    gx = smad_s(s[18], A[18], gx, 3);
    m = mont_m(t);
    gx = smad_s(s[19], A[19], gx, 0);
    gx = smad_s(s[20], A[20], gx, 1);
    const i32 y0s = (i32)(smad_k(m, P, t, 2) >> 32);                // round B's S-box output
    BX_ASSERT_BOUND(iabs64(gx) <= T_DOT && iabs64(y0s) <= B_SBOX, "dot-product group");
    fx = fold64(gx, 3);
    gy = smad_s(s[21], A[21], fy, 0);
    gy = smad_s(s[22], A[22], gy, 1);
    gy = smad_s(s[23], A[23], gy, 2);
    gy = smad_k(y0s, R2, gy + fx, 3);
    BX_ASSERT_BOUND(iabs64(gy) <= T_LAST, "last dot-product group");
    const i32 sig2 = sredc(fold64(gy, 0), 1);
    BX_ASSERT_BOUND(iabs64(sig2) <= B_SIG2, "sig2");
    const i64 c = smulc<1>(sig2, 2);
    constexpr int H = P2_CELLS / 2;
#pragma unroll
    for (int h = 0; h < P2_CELLS; h += H) {
        i64 tt[H];
#pragma unroll
        for (int i = 0; i < H; ++i) {
            if (h + i == 0)
                tt[i] = smad_s(y0s, E[0], add_u32(c, rc[1], 2), 3);
            else
                tt[i] = smad_s(s[h + i], E[h + i], c, i + 2);
        }
#pragma unroll
        for (int i = 0; i < H; ++i)
            if (h + i != 0) tt[i] = smad_s(sig1, A[h + i], tt[i], i + 1);
        sredc_n<H>(tt, s + h);
    }
#pragma unroll
    for (int i = 0; i < P2_CELLS; ++i) BX_ASSERT_BOUND(iabs64(s[i]) <= B_INT, "internal cell");
}

// signed cell -> canonical word (|v| < P)
BX_HD uint32_t canon(i32 v) {
    BX_ASSERT_BOUND(iabs64(v) < (i64)P, "canonicalisation input");
    const uint32_t u = (uint32_t)v;
    return umin(u, u + P);
}

// ---- the parameter table ------------------------------------------------------------------------------------------------
// [0,96) external rounds 0-3 | [96,117) internal rounds | [117,213) external rounds 4-7: round constants * p2_rc_scale(i), canonical
// [216,240) the internal diagonal (Montgomery form) | [240,288) E[24], A[24] of the paired internal rounds (p2_pair_consts)
// [288,672) the FOLDED constants of the external rounds: eight blocks of 24 pairs {K, 0} (a 64-bit addend each), one block per external
//   round's S-boxes in execution order.  Blocks 0, 1, 2 carry rounds 1, 2, 3 and blocks 4, 5, 6 rounds 5, 6, 7; blocks 3 and 7 are zero
//   (behind those S-boxes stand the layers with a change of representation, red64ks_all), so that each external-round loop keeps ONE
//   copy of its S-boxes.  Round 0's constants follow no S-box and round 4's ride in the last internal round: both stay in [0,213).
constexpr int P2_RC_WORDS = 213, P2_DIAG_OFF = 216, P2_PAIR_OFF = P2_DIAG_OFF + P2_CELLS, P2_FOLD_OFF = P2_PAIR_OFF + 2 * P2_CELLS;
constexpr int P2_FOLD_BLOCK = 2 * P2_CELLS, P2_FOLD_BLOCKS = 8, P2_FOLD_WORDS = P2_FOLD_BLOCKS * P2_FOLD_BLOCK;
constexpr int P2_TABLE_WORDS = P2_FOLD_OFF + P2_FOLD_WORDS;
static_assert(P2_DIAG_OFF % 8 == 0 && P2_PAIR_OFF % 8 == 0 && P2_FOLD_OFF % 8 == 0 && (P2_FOLD_BLOCK / 2) % 8 == 0, "the tables are read as 32-byte octets");

// M4 of the external layer and its inverse over F_P (Gauss-Jordan at compile time)
struct P2M4 {
    uint32_t a[4][4];
};
constexpr uint32_t cx_sub(uint32_t a, uint32_t b) { return a >= b ? a - b : a + P - b; }
constexpr P2M4 P2_M4 = {{{5, 7, 1, 3}, {4, 6, 1, 1}, {1, 3, 5, 7}, {1, 1, 4, 6}}};
constexpr P2M4 p2_m4_mul(const P2M4& x, const P2M4& y) {
    P2M4 r = {};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            uint32_t v = 0;
            for (int k = 0; k < 4; ++k) v = (uint32_t)(((uint64_t)x.a[i][k] * y.a[k][j] + v) % P);
            r.a[i][j] = v;
        }
    return r;
}
constexpr P2M4 p2_m4_inverse() {
    uint32_t m[4][8] = {};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 4; ++j) m[i][j] = P2_M4.a[i][j];
        m[i][4 + i] = 1;
    }
    for (int col = 0; col < 4; ++col) {
        int p = col;
        while (p < 3 && m[p][col] == 0) ++p;
        for (int j = 0; j < 8; ++j) {
            const uint32_t v = m[p][j];
            m[p][j] = m[col][j];
            m[col][j] = v;
        }
        const uint32_t inv = cx_pow(m[col][col], P - 2);
        for (int j = 0; j < 8; ++j) m[col][j] = cx_mul(m[col][j], inv);
        for (int i = 0; i < 4; ++i) {
            if (i == col) continue;
            const uint32_t f = m[i][col];
            for (int j = 0; j < 8; ++j) m[i][j] = cx_sub(m[i][j], cx_mul(f, m[col][j]));
        }
    }
    P2M4 r = {};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) r.a[i][j] = m[i][4 + j];
    return r;
}
constexpr bool p2_m4_is_identity(const P2M4& x) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            if (x.a[i][j] != (i == j ? 1u : 0u)) return false;
    return true;
}
static_assert(p2_m4_is_identity(p2_m4_mul(P2_M4, p2_m4_inverse())), "M4^-1");

// the stored constants of the external round that the S-boxes of block b hand their outputs to (nullptr: a zero block)
BX_HD const uint32_t* p2_fold_source(const uint32_t* prm, int b) {
    return (b & 3) == 3 ? nullptr : b < 3 ? prm + (b + 1) * P2_CELLS : prm + 117 + (b - 3) * P2_CELLS;
}
// fold[P2_FOLD_WORDS] from the scaled round constants prm[0, 213).  The stored constants rc' of round r are scaled to the representation
// of the layer output they were added to, which is also that of the S-box outputs in front of the (homogeneous) layer, so
// c = M^-1 rc' on the stored words:  M = circ(2 M4, M4, ..., M4) = (I6 + J6) (x) M4,  M^-1 = (I6 - J6 / 7) (x) M4^-1,  and
// K = c * 2^32 mod P, canonical, as the pair {K, 0}.  Returns whether M c == rc' holds for every folded round (recomputed by the
// layer's definition, not by the inverse).
BX_HD bool p2_fold_consts(const uint32_t* prm, uint32_t* fold) {
    constexpr P2M4 inv = p2_m4_inverse();
    constexpr uint32_t inv7 = cx_pow(7u, P - 2);
    bool ok = true;
    for (int b = 0; b < P2_FOLD_BLOCKS; ++b) {
        uint32_t* out = fold + b * P2_FOLD_BLOCK;
        for (int i = 0; i < P2_FOLD_BLOCK; ++i) out[i] = 0u;
        const uint32_t* rc = p2_fold_source(prm, b);
        if (!rc) continue;
        uint32_t c[P2_CELLS], seventh[4], t[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < 4; ++j) {
            uint64_t sum = 0;
            for (int k = 0; k < P2_CELLS; k += 4) sum += rc[k + j] % P;
            seventh[j] = (uint32_t)(sum % P * inv7 % P);
        }
        for (int k = 0; k < P2_CELLS; k += 4)  // c_k = M4^-1 (rc'_k - (sum of the blocks) / 7)
            for (int i = 0; i < 4; ++i) {
                uint64_t v = 0;
                for (int j = 0; j < 4; ++j) v = ((uint64_t)inv.a[i][j] * ((rc[k + j] % P + P - seventh[j]) % P) + v) % P;
                c[k + i] = (uint32_t)v;
            }
        uint32_t w[P2_CELLS];
        for (int k = 0; k < P2_CELLS; k += 4)  // the layer itself: w_k = M4 c_k, T = sum_k w_k, y_k = w_k + T
            for (int i = 0; i < 4; ++i) {
                uint64_t v = 0;
                for (int j = 0; j < 4; ++j) v += (uint64_t)P2_M4.a[i][j] * c[k + j];
                w[k + i] = (uint32_t)(v % P);
                t[i] = (uint32_t)(((uint64_t)t[i] + w[k + i]) % P);
            }
        for (int i = 0; i < P2_CELLS; ++i) {
            ok = ok && (uint32_t)(((uint64_t)w[i] + t[i & 3]) % P) == rc[i] % P;
            out[2 * i] = (uint32_t)((uint64_t)c[i] * MONT_ONE % P);
        }
    }
    return ok;
}
// the 12 addends of half h (0, 1) of block b as the S-boxes take them
BX_HD void p2_fold_half(const uint32_t* fold, int b, int h, i64* K) {
    const uint32_t* f = fold + b * P2_FOLD_BLOCK + h * P2_CELLS;
    for (int i = 0; i < P2_CELLS / 2; ++i) K[i] = (i64)(((uint64_t)f[2 * i + 1] << 32) | f[2 * i]);
}
// the whole device table from canonical round constants and a canonical diagonal; false if a folded round fails M c == rc'
BX_HD bool p2_build_table(const uint32_t* rc213, const uint32_t* diag24, uint32_t* table) {
    for (int i = 0; i < P2_TABLE_WORDS; ++i) table[i] = 0u;
    // round constants ride in REDC accumulators, pre-scaled to the representation of the round they are added in
    for (int i = 0; i < P2_RC_WORDS; ++i) table[i] = (uint32_t)((uint64_t)(rc213[i] % P) * p2_rc_scale(i) % P);
    for (int i = 0; i < P2_CELLS; ++i) table[P2_DIAG_OFF + i] = fp_encode(diag24[i]);
    i32 pe[P2_CELLS], pa[P2_CELLS];
    p2_pair_consts(table + P2_DIAG_OFF, pe, pa);
    for (int i = 0; i < P2_CELLS; ++i) table[P2_PAIR_OFF + i] = (uint32_t)pe[i], table[P2_PAIR_OFF + P2_CELLS + i] = (uint32_t)pa[i];
    return p2_fold_consts(table, table + P2_FOLD_OFF);
}

// The whole permutation in the exact order and arithmetic of the device kernel (poseidon2.hip: poseidon2_mix); the device
// version differs only in pinning the internal-round sum to v_mad_i64_i32 and in reading the diagonal, the paired rounds'
// constants and the folded external constants from its parameter table (where poseidon2_upload_params put what p2_pair_consts and
// p2_fold_consts derive) into SGPRs.
// prm: [0,96) | [96,117) | [117,213) round constants * p2_rc_scale(i) (canonical), [DIAG..DIAG+24) diagonal (Montgomery).
// Input and output: canonical Montgomery words.  [LO, HI): the live cells, as in the device's poseidon2_mix<LO, HI>: the last layer is
// finished, reduced, made canonical and stored for those cells only, and io[] keeps its input words everywhere else.
// SIGNED_OUT (a sponge that absorbs again, live cells inside the capacity): the live cells are left as the signed words the last
// reduction gave (|v| <= B_CARRY), not made canonical; the next permutation takes them as they are, since the first layer accepts any
// int32.  So the capacity cells of the INPUT are canonical or such carried words; the rate is canonical.
constexpr i64 B_CARRY = (i64)K1_END + (i64)(P / 2) + 60;  // red64ks<K1_END> output (0.555 P)
static_assert(B_CARRY < (i64)P, "carried capacity cells");
template <int DIAG, int LO = 0, int HI = P2_CELLS, bool SIGNED_OUT = false>
BX_HD void poseidon2_mix_bounded(uint32_t* io, const uint32_t* prm) {
    static_assert(!SIGNED_OUT || LO >= 16, "only capacity cells are carried signed");
    i32 s[P2_CELLS];
    i64 y[P2_CELLS], K[P2_CELLS / 2];
    const uint32_t* diag = prm + DIAG;
    for (int i = 0; i < P2_CELLS; ++i) {
        if (i < 16) BX_ASSERT_BOUND(io[i] <= B_IN, "canonical input");
        else BX_ASSERT_BOUND(iabs64((i32)io[i]) <= B_IN, "capacity input: canonical or carried signed");
        s[i] = (i32)io[i];
    }
    uint32_t fold[P2_FOLD_WORDS];  // the device reads these from its parameter table behind the paired rounds' constants
    const bool folded = p2_fold_consts(prm, fold);
    BX_ASSERT_BOUND(folded, "M c == rc' for the folded rounds");
    (void)folded;
    m_ext64s(s, y);
    redc64s_all(y, prm, s);
    for (int r = 0; r < 4; ++r) {
        for (int h = 0; h < 2; ++h) {
            p2_fold_half(fold, r, h, K);
            sbox7s_n<P2_CELLS / 2>(s + h * (P2_CELLS / 2), K);
        }
        m_ext64s(s, y);
        if (r < 3) {
            sredc_all(y, s);
        } else {
            red64ks_all<K1_MID, K2_MID, true>(y, prm[96], s);
            for (int i = 0; i < P2_CELLS; ++i) BX_ASSERT_BOUND(iabs64(s[i]) <= B_MIDOUT, "mid transition output");
        }
    }
    i32 pair_e[P2_CELLS], pair_a[P2_CELLS];  // the device reads these from its parameter table behind the diagonal
    p2_pair_consts(diag, pair_e, pair_a);
    for (int r = 0; r < 20; r += 2) internal_round_pair(s, pair_e, pair_a, prm + 97 + r);
    internal_round<true>(s, diag, prm + 117);
    for (int r = 0; r < 4; ++r) {
        i64 t[4];
        for (int h = 0; h < 2; ++h) {
            p2_fold_half(fold, 4 + r, h, K);
            sbox7s_n<P2_CELLS / 2>(s + h * (P2_CELLS / 2), K);
        }
        m_ext64s_core(s, y, t);
        if (r < 3) {
            m_ext64s_finish(y, t);
            sredc_all(y, s);
        } else {
            m_ext64s_finish<LO, HI>(y, t);
            red64ks_all<K1_END, K2_END, false, LO, HI>(y, 0u, s);
            for (int i = LO; i < HI; ++i) {
                if (SIGNED_OUT) {
                    BX_ASSERT_BOUND(iabs64(s[i]) <= B_CARRY, "carried capacity cell");
                    io[i] = (uint32_t)s[i];
                } else {
                    io[i] = canon(s[i]);
                }
            }
        }
    }
}

}  // inline namespace BX_MAD_FLAVOUR
}  // namespace bx
