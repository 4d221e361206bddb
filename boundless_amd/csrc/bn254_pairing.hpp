// bn254_pairing.hpp — the BN254 optimal-ate pairing on the host, for the Groth16 verifier (groth16_verify.cpp).
//
// Built on the host side of bn254_arith.hpp (Fq, Fq2, XYZZ points; Montgomery form throughout).  Host only: no kernel includes this.
//   Fq6  = Fq2[v] / (v^3 - xi),  xi = 9 + u;   Fq12 = Fq6[w] / (w^2 - v),  so w^6 = xi.
//   As a polynomial in w an Fq12 element is  c0.a0 + c1.a0 w + c0.a1 w^2 + c1.a1 w^3 + c0.a2 w^4 + c1.a2 w^5.
//   The twist is of type D: (x, y) on y^2 = x^3 + 3/xi maps to (x w^2, y w^3) on y^2 = x^3 + 3.
//   Miller loop: optimal ate, loop count 6x + 2 (x = 4965661367192848881) in plain binary, then the lines through pi(Q) and
//   -pi^2(Q).  G2 points run in homogeneous projective coordinates (Costello, Lange, Naehrig: "Faster pairing computations on curves
//   with high-degree twists"); a line is scaled by an Fq2 factor, which the final exponentiation removes.
//   Final exponentiation: f^(q^6 - 1), then ^(q^2 + 1), then the hard part by the addition chain of Fuentes-Castaneda, Knapp and
//   Rodriguez-Henriquez ("Faster hashing to G2"): it raises to c (q^4 - q^2 + 1) / r with c prime to r, which is 1 exactly when the
//   pairing product is.
#pragma once
#include <mutex>

#include "bn254_arith.hpp"

namespace bn {

struct Fq6 {
    Fq2 a0, a1, a2;
};
struct Fq12 {
    Fq6 c0, c1;
};

inline Fq2 fq2_zero() { return {fp_zero<FqP>(), fp_zero<FqP>()}; }
inline Fq2 fq2_one() { return {fq_one(), fp_zero<FqP>()}; }
inline Fq2 conj(const Fq2& a) { return {a.c0, neg(a.c1)}; }
inline Fq2 scale(const Fq2& a, const Fq& k) { return {mul(a.c0, k), mul(a.c1, k)}; }
// a * xi = (9 a0 - a1) + (9 a1 + a0) u
inline Fq2 mul_xi(const Fq2& a) {
    Fq2 t = dbl(dbl(dbl(a)));  // 8 a
    return {sub(add(t.c0, a.c0), a.c1), add(add(t.c1, a.c1), a.c0)};
}
inline Fq2 pow_words(const Fq2& a, const uint32_t* e) {
    Fq2 r = fq2_one();
    for (int i = 255; i >= 0; i--) {
        r = sqr(r);
        if ((e[i >> 5] >> (i & 31)) & 1u) r = mul(r, a);
    }
    return r;
}

// ---- Fq6 ----
inline Fq6 fq6_zero() { return {fq2_zero(), fq2_zero(), fq2_zero()}; }
inline Fq6 fq6_one() { return {fq2_one(), fq2_zero(), fq2_zero()}; }
inline bool is_zero(const Fq6& a) { return is_zero(a.a0) && is_zero(a.a1) && is_zero(a.a2); }
inline bool eq(const Fq6& a, const Fq6& b) { return eq(a.a0, b.a0) && eq(a.a1, b.a1) && eq(a.a2, b.a2); }
inline Fq6 add(const Fq6& a, const Fq6& b) { return {add(a.a0, b.a0), add(a.a1, b.a1), add(a.a2, b.a2)}; }
inline Fq6 sub(const Fq6& a, const Fq6& b) { return {sub(a.a0, b.a0), sub(a.a1, b.a1), sub(a.a2, b.a2)}; }
inline Fq6 neg(const Fq6& a) { return {neg(a.a0), neg(a.a1), neg(a.a2)}; }
inline Fq6 dbl(const Fq6& a) { return {dbl(a.a0), dbl(a.a1), dbl(a.a2)}; }
inline Fq6 mul_v(const Fq6& a) { return {mul_xi(a.a2), a.a0, a.a1}; }
inline Fq6 mul(const Fq6& a, const Fq6& b) {
    Fq2 t0 = mul(a.a0, b.a0), t1 = mul(a.a1, b.a1), t2 = mul(a.a2, b.a2);
    Fq6 r;
    r.a0 = add(t0, mul_xi(sub(sub(mul(add(a.a1, a.a2), add(b.a1, b.a2)), t1), t2)));
    r.a1 = add(sub(sub(mul(add(a.a0, a.a1), add(b.a0, b.a1)), t0), t1), mul_xi(t2));
    r.a2 = add(sub(sub(mul(add(a.a0, a.a2), add(b.a0, b.a2)), t0), t2), t1);
    return r;
}
inline Fq6 sqr(const Fq6& a) { return mul(a, a); }
inline Fq6 scale(const Fq6& a, const Fq2& k) { return {mul(a.a0, k), mul(a.a1, k), mul(a.a2, k)}; }
// a * (b0 + b1 v)
inline Fq6 mul_by_01(const Fq6& a, const Fq2& b0, const Fq2& b1) {
    Fq2 t0 = mul(a.a0, b0), t1 = mul(a.a1, b1);
    Fq6 r;
    r.a0 = add(t0, mul_xi(mul(a.a2, b1)));
    r.a1 = sub(sub(mul(add(a.a0, a.a1), add(b0, b1)), t0), t1);
    r.a2 = add(t1, mul(a.a2, b0));
    return r;
}
inline Fq6 inv(const Fq6& a) {
    Fq2 c0 = sub(sqr(a.a0), mul_xi(mul(a.a1, a.a2)));
    Fq2 c1 = sub(mul_xi(sqr(a.a2)), mul(a.a0, a.a1));
    Fq2 c2 = sub(sqr(a.a1), mul(a.a0, a.a2));
    Fq2 t = inv(add(mul(a.a0, c0), mul_xi(add(mul(a.a2, c1), mul(a.a1, c2)))));
    return {mul(c0, t), mul(c1, t), mul(c2, t)};
}

// ---- Fq12 ----
inline Fq12 fq12_one() { return {fq6_one(), fq6_zero()}; }
inline bool eq(const Fq12& a, const Fq12& b) { return eq(a.c0, b.c0) && eq(a.c1, b.c1); }
inline bool is_one(const Fq12& a) { return eq(a, fq12_one()); }
inline Fq12 mul(const Fq12& a, const Fq12& b) {
    Fq6 t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1);
    return {add(t0, mul_v(t1)), sub(sub(mul(add(a.c0, a.c1), add(b.c0, b.c1)), t0), t1)};
}
inline Fq12 sqr(const Fq12& a) {
    Fq6 ab = mul(a.c0, a.c1);
    return {sub(sub(mul(add(a.c0, a.c1), add(a.c0, mul_v(a.c1))), ab), mul_v(ab)), dbl(ab)};
}
// on the cyclotomic subgroup (after the easy part of the final exponentiation) this is the inverse
inline Fq12 conj(const Fq12& a) { return {a.c0, neg(a.c1)}; }
inline Fq12 inv(const Fq12& a) {
    Fq6 t = inv(sub(sqr(a.c0), mul_v(sqr(a.c1))));
    return {mul(a.c0, t), neg(mul(a.c1, t))};
}
// a * (l0 + l1 w + l3 w^3): the shape of a line of the type-D twist
inline Fq12 mul_by_line(const Fq12& a, const Fq2& l0, const Fq2& l1, const Fq2& l3) {
    Fq6 t0 = scale(a.c0, l0), t1 = mul_by_01(a.c1, l1, l3);
    Fq6 t2 = mul_by_01(add(a.c0, a.c1), add(l0, l1), l3);
    return {add(t0, mul_v(t1)), sub(sub(t2, t0), t1)};
}

// Frobenius constants: g[i] = xi^(i (q - 1) / 6), the factor w^i picks up under x -> x^q; g2[i] = g[i] conj(g[i]) for x -> x^(q^2)
struct FrobConsts {
    Fq2 g[6], g2[6];
};
inline const FrobConsts& frob_consts() {
    static FrobConsts K;
    static std::once_flag once;
    std::call_once(once, [] {
        const uint32_t e[8] = {0x2414d4e1u, 0x34b01759u, 0xe6bda1c2u, 0xee9591c2u, 0xc0403964u, 0xf40d60f3u, 0xd032f006u, 0x0810b7bdu};  // (q - 1) / 6
        Fq2 xi = {to_mont(fp_from<FqP>({9, 0, 0, 0, 0, 0, 0, 0})), fq_one()};
        K.g[0] = fq2_one();
        K.g[1] = pow_words(xi, e);
        for (int i = 2; i < 6; i++) K.g[i] = mul(K.g[i - 1], K.g[1]);
        for (int i = 0; i < 6; i++) K.g2[i] = mul(K.g[i], conj(K.g[i]));
    });
    return K;
}
inline Fq12 frobenius(const Fq12& a) {
    const FrobConsts& K = frob_consts();
    Fq12 r;
    r.c0.a0 = conj(a.c0.a0);
    r.c1.a0 = mul(conj(a.c1.a0), K.g[1]);
    r.c0.a1 = mul(conj(a.c0.a1), K.g[2]);
    r.c1.a1 = mul(conj(a.c1.a1), K.g[3]);
    r.c0.a2 = mul(conj(a.c0.a2), K.g[4]);
    r.c1.a2 = mul(conj(a.c1.a2), K.g[5]);
    return r;
}
inline Fq12 frobenius2(const Fq12& a) {
    const FrobConsts& K = frob_consts();
    Fq12 r;
    r.c0.a0 = a.c0.a0;
    r.c1.a0 = mul(a.c1.a0, K.g2[1]);
    r.c0.a1 = mul(a.c0.a1, K.g2[2]);
    r.c1.a1 = mul(a.c1.a1, K.g2[3]);
    r.c0.a2 = mul(a.c0.a2, K.g2[4]);
    r.c1.a2 = mul(a.c1.a2, K.g2[5]);
    return r;
}

// ---- points ----
// k * p, k an 8-word little-endian number (double-and-add; any k below 2^256)
template <class F>
inline Xyzz<F> scalar_mul(const Aff<F>& p, const uint32_t* k) {
    Xyzz<F> r = xyzz_inf<F>();
    for (int i = 255; i >= 0; i--) {
        r = xyzz_dbl(r);
        if ((k[i >> 5] >> (i & 31)) & 1u) r = xyzz_add_aff(r, p);
    }
    return r;
}
// sum k_i p_i for a handful of points (the verifier's IC sum: at most 65)
template <class F>
inline Xyzz<F> small_msm(const Aff<F>* p, const uint32_t* k, size_t n) {
    Xyzz<F> r = xyzz_inf<F>();
    for (size_t i = 0; i < n; i++) r = xyzz_add(r, scalar_mul(p[i], k + 8 * i));
    return r;
}
// affine, Montgomery coordinates; infinity -> zeros
template <class F>
inline Aff<F> to_affine(const Xyzz<F>& p) {
    Aff<F> r;
    if (is_inf(p)) {
        set_zero(r.x);
        set_zero(r.y);
        return r;
    }
    r.x = mul(p.x, inv(p.zz));
    r.y = mul(p.y, inv(p.zzz));
    return r;
}
// [r] P == O.  G1 has prime order r, so this only matters on the twist, whose group order is r times a cofactor.
inline bool in_g2_subgroup(const Aff<Fq2>& p) {
    uint32_t r[8];
    for (int i = 0; i < 8; i++) r[i] = FrP::m(i);
    return is_inf(scalar_mul(p, r));
}

// ---- Miller loop ----
struct G2Proj {
    Fq2 x, y, z;
};
struct Line {
    Fq2 l0, l1, l3;  // l0 y_P + l1 x_P w + l3 w^3
};
inline Fq2 twist_b3() {  // 3 b', b' = 3 / xi
    Fq2 b;
    curve_b(b);
    return add(dbl(b), b);
}
inline Fq half_mont() {  // 1/2 = (q + 1) / 2, Montgomery form
    return to_mont(fp_from<FqP>({0x6c3e7ea4u, 0x9e10460bu, 0xb438e546u, 0xcbc0b548u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u}));
}
// T <- 2T; the tangent at T
inline Line double_step(G2Proj& t, const Fq& half, const Fq2& b3) {
    Fq2 a = scale(mul(t.x, t.y), half), b = sqr(t.y), c = sqr(t.z);
    Fq2 e = mul(b3, c), f = add(dbl(e), e), g = scale(add(b, f), half);
    Fq2 h = sub(sqr(add(t.y, t.z)), add(b, c)), i = sub(e, b), j = sqr(t.x), e2 = sqr(e);
    t.x = mul(a, sub(b, f));
    t.y = sub(sqr(g), add(dbl(e2), e2));
    t.z = mul(b, h);
    return {neg(h), add(dbl(j), j), i};
}
// T <- T + Q; the line through T and Q (Q affine, not T, not -T)
inline Line add_step(G2Proj& t, const Aff<Fq2>& q) {
    Fq2 theta = sub(t.y, mul(q.y, t.z)), lambda = sub(t.x, mul(q.x, t.z));
    Fq2 c = sqr(theta), d = sqr(lambda), e = mul(lambda, d), f = mul(t.z, c), g = mul(t.x, d);
    Fq2 h = sub(add(e, f), dbl(g));
    Fq2 j = sub(mul(theta, q.x), mul(lambda, q.y));
    t.x = mul(lambda, h);
    t.y = sub(mul(theta, sub(g, h)), mul(e, t.y));
    t.z = mul(t.z, e);
    return {lambda, neg(theta), j};
}
inline Fq12 eval_line(const Fq12& f, const Line& l, const Aff<Fq>& p) { return mul_by_line(f, scale(l.l0, p.y), scale(l.l1, p.x), l.l3); }

// prod_i miller(P_i, Q_i) with one accumulator.  Points are affine, Montgomery, on their curves, the Q_i in the r-order subgroup;
// a pair with either point at infinity contributes 1.  n <= 68 (the verifier passes 4).
inline Fq12 multi_miller_loop(const Aff<Fq>* ps, const Aff<Fq2>* qs, size_t n) {
    constexpr size_t MAXP = 68;
    const Aff<Fq>* p[MAXP];
    const Aff<Fq2>* q[MAXP];
    G2Proj t[MAXP];
    size_t m = 0;
    for (size_t i = 0; i < n && m < MAXP; i++) {
        if (aff_is_inf(ps[i]) || aff_is_inf(qs[i])) continue;
        p[m] = &ps[i];
        q[m] = &qs[i];
        t[m] = {qs[i].x, qs[i].y, fq2_one()};
        m++;
    }
    Fq12 f = fq12_one();
    if (m == 0) return f;
    const Fq half = half_mont();
    const Fq2 b3 = twist_b3();
    const uint64_t low = 0x9d797039be763ba8ull;  // 6x + 2 = 2^64 + low
    for (int i = 63; i >= 0; i--) {
        f = sqr(f);
        for (size_t k = 0; k < m; k++) f = eval_line(f, double_step(t[k], half, b3), *p[k]);
        if ((low >> i) & 1u)
            for (size_t k = 0; k < m; k++) f = eval_line(f, add_step(t[k], *q[k]), *p[k]);
    }
    const FrobConsts& K = frob_consts();
    for (size_t k = 0; k < m; k++) {
        // pi(Q) = (conj(x) xi^((q-1)/3), conj(y) xi^((q-1)/2)); -pi^2(Q) = (x xi^((q^2-1)/3), -y xi^((q^2-1)/2))
        Aff<Fq2> q1 = {mul(conj(q[k]->x), K.g[2]), mul(conj(q[k]->y), K.g[3])};
        Aff<Fq2> q2 = {mul(q[k]->x, K.g2[2]), neg(mul(q[k]->y, K.g2[3]))};
        f = eval_line(f, add_step(t[k], q1), *p[k]);
        f = eval_line(f, add_step(t[k], q2), *p[k]);
    }
    return f;
}

// f^x on the cyclotomic subgroup, x = 4965661367192848881
inline Fq12 pow_x(const Fq12& a) {
    const uint64_t x = 4965661367192848881ull;
    Fq12 r = a;
    for (int i = 61; i >= 0; i--) {  // x has 63 bits
        r = sqr(r);
        if ((x >> i) & 1u) r = mul(r, a);
    }
    return r;
}
inline Fq12 final_exponentiation(const Fq12& f) {
    Fq12 r = mul(conj(f), inv(f));  // ^(q^6 - 1); f is never 0: a product of non-zero line values
    r = mul(frobenius2(r), r);      // ^(q^2 + 1)
    auto nx = [](const Fq12& a) { return conj(pow_x(a)); };  // a^(-x)
    Fq12 y0 = nx(r), y1 = sqr(y0), y2 = sqr(y1), y3 = mul(y2, y1), y4 = nx(y3), y5 = sqr(y4), y6 = nx(y5);
    y3 = conj(y3);
    y6 = conj(y6);
    Fq12 y7 = mul(y6, y4), y8 = mul(y7, y3), y9 = mul(y8, y1), y10 = mul(y8, y4), y11 = mul(y10, r);
    Fq12 y13 = mul(frobenius(y9), y11), y14 = mul(frobenius2(y8), y13);
    Fq12 y15 = frobenius(frobenius2(mul(conj(r), y9)));
    return mul(y15, y14);
}
// prod e(P_i, Q_i) == 1
inline bool pairing_product_is_one(const Aff<Fq>* ps, const Aff<Fq2>* qs, size_t n) {
    return is_one(final_exponentiation(multi_miller_loop(ps, qs, n)));
}

}  // namespace bn
