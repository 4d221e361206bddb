// bn254_edge_ops.hpp — the one op table of the BN254 edge-operand checks (tests/bn254_edge.py): every call into
// boundless_amd/csrc/bn254_arith.hpp that those checks make goes through apply_*() below, so the host program
// (bn254_edge_host.cpp) and the device module (bn254_edge_dev.hip) run the same text.
//
// A record is a row of u32 words; word 0 is the op.  Field elements are the stored limb patterns (Montgomery form, 8 words).
//   field (Fq, Fr):  in  [op, a(8), b(8), e_lo, e_hi]                       out [r(8), flag]
//   Fq2:             in  [op, a(16), b(16)]                                 out [r(16)]
//   curve over F (E = words of F): in [op, k, P: x y zz zzz (4E), Q: x y zz zzz (4E)]   out [x(E), y(E), flag]
//     the curve ops answer through to_affine_canonical (canonical coordinates, infinity as zeros); flag = the result is infinity
//     (ON_CURVE: flag = on_curve(Q.x, Q.y), coordinates zero).  Affine operands are Q.x, Q.y.
#pragma once
#include "bn254_arith.hpp"

namespace bn_edge {

using namespace bn;

enum Family : uint32_t { FIELD_Q = 0, FIELD_R = 1, FQ2 = 2, CURVE_Q = 3, CURVE_Q2 = 4, N_FAMILIES = 5 };
enum FieldOp : uint32_t { F_ADD, F_SUB, F_NEG, F_DBL, F_MUL, F_SQR, F_TO_MONT, F_FROM_MONT, F_INV, F_POW, F_IS_ZERO, F_EQ, F_GE_MOD };
enum Fq2Op : uint32_t { E_ADD, E_SUB, E_NEG, E_DBL, E_MUL, E_SQR, E_INV, E_TO_MONT, E_FROM_MONT };
enum CurveOp : uint32_t { C_ROUNDTRIP, C_AFF_DBL, C_XYZZ_DBL, C_ADD_AFF, C_ADD, C_MUL_SMALL, C_ON_CURVE };

constexpr uint32_t FIELD_IN = 19, FIELD_OUT = 9, FQ2_IN = 33, FQ2_OUT = 16;
template <class F>
struct CurveWords {
    static constexpr uint32_t E = sizeof(F) / 4, IN = 2 + 8 * E, OUT = 2 * E + 1;
};

BN_HD uint32_t words_in(uint32_t family) {
    return family <= FIELD_R ? FIELD_IN : family == FQ2 ? FQ2_IN : family == CURVE_Q ? CurveWords<Fq>::IN : CurveWords<Fq2>::IN;
}
BN_HD uint32_t words_out(uint32_t family) {
    return family <= FIELD_R ? FIELD_OUT : family == FQ2 ? FQ2_OUT : family == CURVE_Q ? CurveWords<Fq>::OUT : CurveWords<Fq2>::OUT;
}

template <class P>
BN_HD Fp<P> ld(const uint32_t* w) {
    Fp<P> a;
    for (int i = 0; i < 8; i++) a.v[i] = w[i];
    return a;
}
template <class P>
BN_HD void st(uint32_t* w, const Fp<P>& a) {
    for (int i = 0; i < 8; i++) w[i] = a.v[i];
}
BN_HD void ld_f(const uint32_t* w, Fq& a) { a = ld<FqP>(w); }
BN_HD void ld_f(const uint32_t* w, Fq2& a) {
    a.c0 = ld<FqP>(w);
    a.c1 = ld<FqP>(w + 8);
}
BN_HD void st_f(uint32_t* w, const Fq& a) { st(w, a); }
BN_HD void st_f(uint32_t* w, const Fq2& a) {
    st(w, a.c0);
    st(w + 8, a.c1);
}
BN_HD Fq mont_one(const Fq&) { return fq_one(); }
BN_HD Fr mont_one(const Fr&) { return fr_one(); }

template <class P>
BN_HD void apply_field(const uint32_t* in, uint32_t* out) {
    const Fp<P> a = ld<P>(in + 1), b = ld<P>(in + 9);
    const uint64_t e = (uint64_t)in[17] | ((uint64_t)in[18] << 32);
    Fp<P> r = fp_zero<P>();
    uint32_t flag = 0;
    switch (in[0]) {
        case F_ADD: r = add(a, b); break;
        case F_SUB: r = sub(a, b); break;
        case F_NEG: r = neg(a); break;
        case F_DBL: r = dbl(a); break;
        case F_MUL: r = mul(a, b); break;
        case F_SQR: r = sqr(a); break;
        case F_TO_MONT: r = to_mont(a); break;
        case F_FROM_MONT: r = from_mont(a); break;
        case F_INV: r = inv(a); break;
        case F_POW: r = pow_u64(a, e, mont_one(a)); break;
        case F_IS_ZERO: flag = is_zero(a); break;
        case F_EQ: flag = eq(a, b); break;
        case F_GE_MOD: flag = ge_mod<P>(in + 1); break;
        default: flag = 0xdeadu; break;
    }
    st(out, r);
    out[8] = flag;
}

BN_HD void apply_fq2(const uint32_t* in, uint32_t* out) {
    Fq2 a, b, r;
    ld_f(in + 1, a);
    ld_f(in + 17, b);
    set_zero(r);
    switch (in[0]) {
        case E_ADD: r = add(a, b); break;
        case E_SUB: r = sub(a, b); break;
        case E_NEG: r = neg(a); break;
        case E_DBL: r = dbl(a); break;
        case E_MUL: r = mul(a, b); break;
        case E_SQR: r = sqr(a); break;
        case E_INV: r = inv(a); break;
        case E_TO_MONT: r = to_mont(a); break;
        case E_FROM_MONT: r = from_mont(a); break;
        default: break;
    }
    st_f(out, r);
}

template <class F>
BN_HD void apply_curve(const uint32_t* in, uint32_t* out) {
    constexpr uint32_t E = CurveWords<F>::E;
    Xyzz<F> p, q;
    ld_f(in + 2, p.x);
    ld_f(in + 2 + E, p.y);
    ld_f(in + 2 + 2 * E, p.zz);
    ld_f(in + 2 + 3 * E, p.zzz);
    ld_f(in + 2 + 4 * E, q.x);
    ld_f(in + 2 + 5 * E, q.y);
    ld_f(in + 2 + 6 * E, q.zz);
    ld_f(in + 2 + 7 * E, q.zzz);
    const Aff<F> qa = {q.x, q.y};
    Xyzz<F> r = xyzz_inf<F>();
    bool answered = false;
    uint32_t flag = 0;
    switch (in[0]) {
        case C_ROUNDTRIP: r = from_aff(qa); break;
        case C_AFF_DBL: r = aff_dbl(qa); break;
        case C_XYZZ_DBL: r = xyzz_dbl(p); break;
        case C_ADD_AFF: r = xyzz_add_aff(p, qa); break;
        case C_ADD: r = xyzz_add(p, q); break;
        case C_MUL_SMALL: r = xyzz_mul_small(p, in[1]); break;
        case C_ON_CURVE:
            flag = on_curve(qa);
            answered = true;
            break;
        default: break;
    }
    Aff<F> a;
    set_zero(a.x);
    set_zero(a.y);
    if (!answered) {
        a = to_affine_canonical(r);
        flag = is_inf(r);
    }
    st_f(out, a.x);
    st_f(out + E, a.y);
    out[2 * E] = flag;
}

BN_HD void apply(uint32_t family, const uint32_t* in, uint32_t* out) {
    switch (family) {
        case FIELD_Q: apply_field<FqP>(in, out); break;
        case FIELD_R: apply_field<FrP>(in, out); break;
        case FQ2: apply_fq2(in, out); break;
        case CURVE_Q: apply_curve<Fq>(in, out); break;
        default: apply_curve<Fq2>(in, out); break;
    }
}

}  // namespace bn_edge
