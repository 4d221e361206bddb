// lazy_ext.hpp — weighted sums over Fp4 without a reduction per product, on the signed arithmetic of poseidon2_arith.hpp:
//   LazyExtAcc       sum_k w_k * x_k,  w_k in Fp4 (a wave-uniform weight: a mix power, a power of the evaluation point), x_k in Fp
//   WeightedExtAcc   sum_k W_k * V_k,  W_k in Fp4 (wave-uniform, centred), V_k in Fp4 (lane-varying): the ext-valued constraints of an
//                    eval_check under their mix powers
//   f4_mul_cc        one ext x ext product of centred operands
// and the values of the synthetic circuit's ext-valued constraints that WeightedExtAcc sums (accumulator_value, pair_value).
//
// The canonical form of the first (f4_scale + f4_add) costs 4 x (5 + 3) = 32 VALU instructions per term; mix_poly_coeffs,
// batch_evaluate_any and the mixing of eval_check are nothing else, which made these "streaming" entry points VALU-bound
// (mix_poly_coeffs 3.0 TB/s, batch_evaluate_any 2.5 TB/s in round 1).  The canonical form of the second (f4_mul + f4_add) costs 19
// products, each with a reduction and a conditional subtraction: 69 multiply-class and 74 other instructions per term.
//
// Both accumulators are 64-bit CHAINS that are never reduced on the way (2^63 = 2.2755 P^2).  Where a chain would leave 64 bits it is
// FOLDED, a = hi * 2^32 + lo -> hi * R + lo (fold_r; R = 2^32 mod P = 0.1334 P, so the value is congruent mod P and
// |result| <= fold_ub(|a|) = |a|/16 + 2^32 + R): one multiply-add and the copy that puts lo beside a zero register.
//   LazyExtAcc      weights centred once where their table is built (|w| <= P/2); x canonical (add: a term <= P^2/2) or centred
//                   (add_centred: <= P^2/4).  One chain per component, folded before the term that would take the products since the
//                   last fold beyond 8 (P/2)^2 = 2 P^2:  A <= fold_ub(A) + 2 P^2, A <= 2.134 P^2 — every fourth add, every eighth
//                   add_centred, any mixture of the two.  finish: canon(sredc(fold_r(A))), fold_ub(A) <= 0.134 P^2 <= FINAL_MAX.
//                   4 multiply-adds + 8/4 per term instead of 32 instructions.
//   WeightedExtAcc  |W| <= P/2, |V| <= P (a canonical word, or a sredc result: no centring of the lane values).  The 16 raw products of a
//                   term go into the SEVEN coefficients of the polynomial product W(X) V(X); coefficient m takes min(m, 6 - m) + 1
//                   products of <= P^2/2 per term and is folded after every term (m = 2, 3, 4: A <= fold_ub(A) + 2 P^2), every second
//                   (m = 1, 5) or every fourth (m = 0, 6).  The wrap by X^4 = -11 and the reductions happen once, in finish:
//                   u_m = sredc(fold_r(C_{m+4})), |u| <= 0.57 P;  out_m = canon(sredc(fold_r(C_m) + NB * u_m)),
//                   the operand <= 0.134 P^2 + 0.467 * 0.57 P^2 = 0.40 P^2 <= FINAL_MAX.  16 multiply-adds + 9 per term.
// Every step is a congruence mod P with the same power of 2^-32 as fp_mul (one sredc between the raw products and the result), so the
// results equal the canonical forms bit for bit.  The bounds are static_asserts below; the host build (BX_CHECK_BOUNDS) asserts every
// fold operand, every chain after every term and the operand of every reduction (tests/host_arith_check.cpp, tests/ext_mix_check.cpp).
#pragma once
#include "fp.hpp"
#include "poseidon2_arith.hpp"

namespace bx {
inline namespace BX_MAD_FLAVOUR {

// largest sredc operand whose result is < P in magnitude: ub(FINAL_MAX) = P - 1
constexpr i64 FINAL_MAX = ((i64)(P / 2) - 1) * ((i64)1 << 32);
static_assert(ub(FINAL_MAX) < (i64)P && FINAL_MAX <= SREDC_MAX, "FINAL_MAX");

// r * R + c: the product inside fold_r, and a term of a G = 1 sum (the lone factor times the Montgomery one).  In a translation unit
// that leaves its multiply-adds to the compiler (BX_PLAIN_MAD) the device build multiplies by an opaque copy of R, one per use: with the
// constant in sight hipcc rewrites a sum of r_i * R as (sum of r_i) * R, sign-extends every r_i, adds them in 64 bits and emulates a
// 64 x 32-bit product, and it takes a single r * R apart into shifts.  The copy lives in an SGPR (an s_mov per use, no VALU work), is
// signed so that the product stays a v_mad_i64_i32 (an opaque unsigned word gets an emulated v_mad_u64_u32 product), and comes out of a
// volatile asm (CSE merges the copies of a plain one and the rewrite is back).  Same 64-bit integer either way.
BX_HD i64 smad_r(i32 r, i64 c, int alt = 0) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(BX_PLAIN_MAD)
    (void)alt;
    i32 k = (i32)MONT_ONE;
    asm volatile("" : "+s"(k));
    return (i64)r * (i64)k + c;
#else
    return smad_k(r, MONT_ONE, c, alt);
#endif
}

// a -> hi(a) * R + lo(a) with lo unsigned: congruent to a mod P since 2^32 == R, and |result| <= |a|/16 + 2^32 + R.  One multiply-add,
// by smad_r's opaque signed copy of R where the multiply-adds are the compiler's: one v_mad_i64_i32 whose addend is (lo, 0).
BX_HD i64 fold_r(i64 a, int alt = 0) {
    BX_ASSERT_BOUND(a >= -INT64_MAX, "fold_r operand");
    const i64 r = smad_r((i32)(a >> 32), (i64)(uint32_t)a, alt);
    BX_ASSERT_BOUND(iabs64(r) <= iabs64(a) / 16 + ((i64)1 << 32) + (i64)MONT_ONE, "fold_r result");
    return r;
}
// a * b + c, a step of a chain.  The device build of a BX_PLAIN_MAD translation unit hides the result from the optimiser (an empty asm, no
// instruction): left in sight, hipcc reassociates fold + t1 + ... + t5 into fold + (t1 + ... + t5), sums the terms in a chain of their own
// and pays a 64-bit add per segment to bring the fold in; hidden, every step is the one v_mad_i64_i32 whose addend is the chain.
BX_HD i64 smad_chain(i32 a, i32 b, i64 c, int alt = 0) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(BX_PLAIN_MAD)
    (void)alt;
    i64 r = (i64)a * (i64)b + c;
    asm("" : "+v"(r));
    return r;
#else
    return smad(a, b, c, alt);
#endif
}
// the bound of a chain that is folded before or after every `rest` of new terms, however long it runs: fold_ub(A) <= A/16 + R + 2^32, so
// 16/15 of the rest holds
constexpr i64 chain_steady(i64 rest) { return (rest + (i64)MONT_ONE + ((i64)1 << 32)) / 15 * 16 + 16; }

// ---- ext x ext product on the signed lazy arithmetic: 40 multiply-class instructions instead of the 69 (+62 cheap ones) of
// fp.hpp's f4_mul, which reduces and conditionally subtracts after every one of its 19 base products.  Operands are CENTRED
// (|.| <= P/2), so four raw products fit one 64-bit accumulator (4 (P/2)^2 = P^2 <= SREDC_MAX = 1.2 P^2): every output
// component is one accumulation of its <= 4 products plus NBETA times the (once reduced) wrapped-around part, and one
// reduction.  Bounds (rho = P/2^32 = 0.469): u = sredc(<= 3 products) has |u| <= 0.75 rho P + P/2 = 0.85 P, |NB| = 0.467 P, so the
// largest accumulator is component 2's: 3 (P/2)^2 + 0.467 P * 0.617 P = 1.04 P^2.  Result canonical; congruent to f4_mul.
struct C4 {
    i32 c[4];
};
constexpr i32 NBETA_C = (i32)MONT_NBETA - (i32)P;  // Montgomery form of -11, centred
BX_HD C4 f4_centre(const Fp4& a) { return C4{{fp_centre(a.c[0]), fp_centre(a.c[1]), fp_centre(a.c[2]), fp_centre(a.c[3])}}; }
BX_HD Fp4 f4_mul_cc(const C4& a, const C4& b) {
    constexpr i32 NB = NBETA_C;
    const i64 t3 = smad(a.c[0], b.c[3], smad(a.c[1], b.c[2], smad(a.c[2], b.c[1], smul(a.c[3], b.c[0]))));
    const i32 u2 = sredc(smul(a.c[3], b.c[3]));
    const i64 t2 = smad(NB, u2, smad(a.c[0], b.c[2], smad(a.c[1], b.c[1], smul(a.c[2], b.c[0]))));
    const i32 u1 = sredc(smad(a.c[2], b.c[3], smul(a.c[3], b.c[2])));
    const i64 t1 = smad(NB, u1, smad(a.c[0], b.c[1], smul(a.c[1], b.c[0])));
    const i32 u0 = sredc(smad(a.c[1], b.c[3], smad(a.c[2], b.c[2], smul(a.c[3], b.c[1]))));
    const i64 t0 = smad(NB, u0, smul(a.c[0], b.c[0]));
    return Fp4{{canon(sredc(t0)), canon(sredc(t1)), canon(sredc(t2)), canon(sredc(t3))}};
}
BX_HD Fp4 f4_mul_lz(const Fp4& a, const Fp4& b) { return f4_mul_cc(f4_centre(a), f4_centre(b)); }  // canonical in, canonical out

// ---- sum_k w_k * x_k: ext weight x base value ----
struct LazyExtAcc {
    static constexpr i64 UNIT = (i64)(P / 2) * (i64)(P / 2);  // an add_centred term; an add term (x canonical) is at most two of them
    static constexpr int UNITS = 8;                            // what a chain takes between two folds
    static constexpr i64 STEADY = chain_steady(UNITS * UNIT + 2 * (i64)P);  // + 2P: P/2 * (P - 1) against 2 UNIT
    static_assert(STEADY < INT64_MAX && fold_ub(STEADY) + UNITS * UNIT + 2 * (i64)P <= STEADY, "LazyExtAcc: the chain bound is not invariant below 2^63");
    static_assert(fold_ub(STEADY) <= FINAL_MAX, "LazyExtAcc: the folded chain beyond the last reduction's range");
    i64 a[4];
    int n;  // units since the last fold
    BX_HD void reset() {
        for (int c = 0; c < 4; ++c) a[c] = 0;
        n = 0;
    }
    BX_HD void fold() {
        for (int c = 0; c < 4; ++c) a[c] = fold_r(a[c], c);
        n = 0;
    }
    // w and x both centred (|.| <= P/2): a term of one unit
    BX_HD void add_centred(const i32 w[4], i32 xc) {
        BX_ASSERT_BOUND(iabs64(xc) <= (i64)(P / 2), "LazyExtAcc: a value that is not centred");
        if (n + 1 > UNITS) fold();
        for (int c = 0; c < 4; ++c) {
            BX_ASSERT_BOUND(iabs64(w[c]) <= (i64)(P / 2), "LazyExtAcc: a weight that is not centred");
            a[c] = smad_chain(w[c], xc, a[c], c);
            BX_ASSERT_BOUND(iabs64(a[c]) <= STEADY, "LazyExtAcc chain");
        }
        n += 1;
    }
    // w: centred weight (|w[c]| <= P/2), x: canonical: a term of two units
    BX_HD void add(const i32 w[4], uint32_t x) {
        BX_ASSERT_BOUND(x < P, "LazyExtAcc: a value that is not canonical");
        if (n + 2 > UNITS) fold();
        for (int c = 0; c < 4; ++c) {
            BX_ASSERT_BOUND(iabs64(w[c]) <= (i64)(P / 2), "LazyExtAcc: a weight that is not centred");
            a[c] = smad_chain(w[c], (i32)x, a[c], c);
            BX_ASSERT_BOUND(iabs64(a[c]) <= STEADY, "LazyExtAcc chain");
        }
        n += 2;
    }
    BX_HD Fp4 finish() {
        Fp4 r;
        for (int c = 0; c < 4; ++c) {
            const i64 t = fold_r(a[c], c);
            BX_ASSERT_BOUND(iabs64(t) <= FINAL_MAX, "LazyExtAcc folded chain");
            r.c[c] = canon(sredc(t, c));
        }
        return r;
    }
};

// ---- sum_k W_k * V_k: ext weight x ext value ----
constexpr int wx_products(int m) { return (m < 3 ? m : 6 - m) + 1; }  // of a term, into coefficient m of the polynomial product
constexpr int wx_period(int m) { return 4 / wx_products(m); }         // terms between two folds of coefficient m: 4, 2, 1, 1, 1, 2, 4
struct WeightedExtAcc {
    static constexpr i64 BW = (i64)(P / 2), BV = (i64)P;       // |W[c]| <= P/2 (centred), |V[c]| <= P
    static constexpr i64 PROD = BW * BV;
    static constexpr int products(int m) { return wx_products(m); }
    static constexpr int period(int m) { return wx_period(m); }
    static constexpr i64 REST = 4 * PROD;                       // the most any coefficient takes between two folds
    static constexpr i64 STEADY = chain_steady(REST);
    static_assert(wx_products(0) * wx_period(0) <= 4 && wx_products(1) * wx_period(1) <= 4 && wx_products(2) * wx_period(2) <= 4 && wx_products(3) * wx_period(3) <= 4,
                  "WeightedExtAcc: a coefficient takes more than four products between two folds");
    static_assert(STEADY < INT64_MAX && fold_ub(STEADY) + REST <= STEADY, "WeightedExtAcc: the chain bound is not invariant below 2^63");
    static constexpr i64 B_U = ub(fold_ub(STEADY));             // the wrapped-around part, reduced
    static constexpr i64 T_OUT = fold_ub(STEADY) + (i64)(-NBETA_C) * B_U;
    static_assert(fold_ub(STEADY) <= SREDC_MAX && T_OUT <= FINAL_MAX, "WeightedExtAcc: a component beyond the last reduction's range");
    i64 c[7];
    int n;  // terms
    BX_HD void reset() {
        for (int m = 0; m < 7; ++m) c[m] = 0;
        n = 0;
    }
    BX_HD void add(const i32 w[4], const i32 v[4]) {
        for (int k = 0; k < 4; ++k) {
            BX_ASSERT_BOUND(iabs64(w[k]) <= BW, "WeightedExtAcc: a weight that is not centred");
            BX_ASSERT_BOUND(iabs64(v[k]) <= BV, "WeightedExtAcc: a value beyond P");
        }
        // by columns of the product, so that consecutive steps belong to different chains
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i + j] = smad_chain(v[j], w[i], c[i + j], i);
        ++n;
#pragma unroll
        for (int m = 0; m < 7; ++m) {
            BX_ASSERT_BOUND(iabs64(c[m]) <= STEADY, "WeightedExtAcc chain");
            if (period(m) == 1 || n % period(m) == 0) c[m] = fold_r(c[m], m);
        }
    }
    BX_HD Fp4 finish() {
        Fp4 r;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            i64 t = fold_r(c[m], m);
            if (m < 3) {
                const i32 u = sredc(fold_r(c[m + 4], m + 1), m);
                BX_ASSERT_BOUND(iabs64(u) <= B_U, "WeightedExtAcc wrapped part");
                t = smad(NBETA_C, u, t, m);
            }
            BX_ASSERT_BOUND(iabs64(t) <= T_OUT, "WeightedExtAcc component");
            r.c[m] = canon(sredc(t, m));
        }
        return r;
    }
};

// ---- the ext-valued constraints of the synthetic circuit (circuit.hip's eval_check), as values for a WeightedExtAcc ----
// What a domain point shares between its constraints: the selectors `first` and `last`, centred once.
struct TailSelectors {
    i32 fm1;    // first - 1, centred
    i64 nfr;    // -first * R with first centred: <= P/2 * R
    i32 last;   // centred
};
BX_HD TailSelectors tail_selectors(uint32_t first, uint32_t last) {
    return TailSelectors{fp_centre(fp_sub(first, MONT_ONE)), smad_r(-fp_centre(first), 0), fp_centre(last)};
}
// An accumulator's constraint  a - inner * fac,  inner = ab * (1 - first) + first (the running product one row back, or 1 on the first
// row),  fac = beta + x.  a, ab, x: canonical words as loaded; beta: centred (wave-uniform).  All of it stays unreduced:
//   -inner_k   = sredc(ab_k * (first - 1) [- first * R])                   operand <= P * P/2 + P/2 * R = 0.567 P^2,  |.| <= 0.766 P
//   fac        = (beta_0 + centre(x), beta_1, beta_2, beta_3)              |fac_0| <= P,  the others <= P/2
//   wrapped    u_m = sredc(sum_{i+j=m+4} -inner_i * fac_j)                 <= 3 products without fac_0: 1.149 P^2 <= SREDC_MAX
//   v_m        = sredc(fold_r(sum_{i+j=m} -inner_i * fac_j + NB * u_m + a_m * R))     the sum <= 2.05 P^2 < 2^63,  |v| <= 0.57 P
// v_m == (a - inner * fac)_m as Montgomery words, |v_m| <= P as WeightedExtAcc asks.
constexpr i64 B_NINNER = ub((i64)P * (i64)(P / 2) + (i64)(P / 2) * (i64)MONT_ONE);
constexpr i64 B_FAC0 = 2 * (i64)(P / 2), B_FACK = (i64)(P / 2);
constexpr i64 T_ACC_WRAP = 3 * B_NINNER * B_FACK;
constexpr i64 acc_component(int m) {  // the sum behind v_m: one product with fac_0, m without, the wrapped part of 3 - m products, a_m * R
    return B_NINNER * B_FAC0 + m * B_NINNER * B_FACK + (m < 3 ? (i64)(-NBETA_C) * ub((3 - m) * B_NINNER * B_FACK) : (i64)0) + (i64)P * (i64)MONT_ONE;
}
constexpr i64 B_ACC_U = ub(T_ACC_WRAP);
constexpr i64 T_ACC_OUT = acc_component(3);  // the largest: 2.05 P^2
static_assert(T_ACC_WRAP <= SREDC_MAX, "accumulator_value: the wrapped part beyond sredc's range");
static_assert(acc_component(0) <= T_ACC_OUT && acc_component(1) <= T_ACC_OUT && acc_component(2) <= T_ACC_OUT, "accumulator_value: component 3 is not the largest");
static_assert(T_ACC_OUT < INT64_MAX - T_ACC_OUT / 64 && fold_ub(T_ACC_OUT) <= SREDC_MAX && ub(fold_ub(T_ACC_OUT)) <= WeightedExtAcc::BV,
              "accumulator_value: a component leaves 64 bits or the accumulator's value bound");
BX_HD void accumulator_value(const Fp4& a, const Fp4& ab, const TailSelectors& sel, const i32 beta[4], uint32_t x, i32 v[4]) {
    i32 ni[4], f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        BX_ASSERT_BOUND(a.c[k] < P && ab.c[k] < P && iabs64(beta[k]) <= (i64)(P / 2), "accumulator_value operands");
        ni[k] = sredc(smad((i32)ab.c[k], sel.fm1, k == 0 ? sel.nfr : (i64)0, k), k);
        BX_ASSERT_BOUND(iabs64(ni[k]) <= B_NINNER, "accumulator_value inner");
        f[k] = beta[k];
    }
    f[0] += fp_centre(x);
    const i32 u2 = sredc(smul(ni[3], f[3]));
    const i32 u1 = sredc(smad_chain(ni[2], f[3], smul(ni[3], f[2])));
    const i32 u0 = sredc(smad_chain(ni[1], f[3], smad_chain(ni[2], f[2], smul(ni[3], f[1]))));
    BX_ASSERT_BOUND(iabs64(u0) <= B_ACC_U && iabs64(u1) <= B_ACC_U && iabs64(u2) <= B_ACC_U, "accumulator_value wrapped part");
    i64 t[4];
    t[3] = smad_chain(ni[0], f[3], smad_chain(ni[1], f[2], smad_chain(ni[2], f[1], smul(ni[3], f[0]))));
    t[2] = smad_chain(NBETA_C, u2, smad_chain(ni[0], f[2], smad_chain(ni[1], f[1], smul(ni[2], f[0]))));
    t[1] = smad_chain(NBETA_C, u1, smad_chain(ni[0], f[1], smul(ni[1], f[0])));
    t[0] = smad_chain(NBETA_C, u0, smul(ni[0], f[0]));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t[k] = smad_r((i32)a.c[k], t[k], k);
        BX_ASSERT_BOUND(iabs64(t[k]) <= T_ACC_OUT, "accumulator_value component");
        v[k] = sredc(fold_r(t[k], k), k);
    }
}
// A permutation pair's closing constraint  last * (hi - lo)  over the two running products' last rows: the difference of two canonical
// words (|d| < P) times the centred selector, operand <= P * P/2, |v| <= 0.734 P.
static_assert((i64)P * (i64)(P / 2) <= SREDC_MAX && ub((i64)P * (i64)(P / 2)) <= WeightedExtAcc::BV, "pair_value");
BX_HD void pair_value(const Fp4& hi, const Fp4& lo, const TailSelectors& sel, i32 v[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        BX_ASSERT_BOUND(hi.c[k] < P && lo.c[k] < P, "pair_value operands");
        v[k] = sredc(smul((i32)hi.c[k] - (i32)lo.c[k], sel.last, k), k);
    }
}

}  // inline namespace BX_MAD_FLAVOUR
}  // namespace bx
