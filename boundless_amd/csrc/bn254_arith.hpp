// bn254_arith.hpp — BN254 field and curve arithmetic for the Groth16 prover (bn254.hip), host and device.
//
// Conventions (the Groth16 conventions block is in groth16.hpp):
//   Fq, Fr: 8 x u32 little-endian limbs, Montgomery form with R = 2^256, CIOS multiplication.  Every operation returns a fully
//   reduced value (< modulus), so equality and zero tests are limb compares.  Fq2 = Fq[u] / (u^2 + 1), stored c0 then c1.
//   G1: y^2 = x^3 + 3 over Fq; G2: y^2 = x^3 + 3/(9+u) over Fq2 (pinned by the reference vector).
//   Affine points in memory: x then y; the point at infinity is all zeros.  Accumulators are XYZZ (x = X/ZZ, y = Y/ZZZ, ZZ^3 = ZZZ^2);
//   ZZ = 0 is infinity.  Additions handle the doubling (P + P) and the inverse (P + (-P)) cases explicitly.
// Plain C++ on 64-bit products (hipcc emits v_mad_u64_u32 carry chains); no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bn {

#define BN_HD __host__ __device__ __forceinline__

struct FqP {
    static BN_HD uint32_t m(int j) {
        constexpr uint32_t M[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
        return M[j];
    }
    static constexpr uint32_t INV = 0xe4866389u;  // -q^-1 mod 2^32
};
struct FrP {
    static BN_HD uint32_t m(int j) {
        constexpr uint32_t M[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
        return M[j];
    }
    static constexpr uint32_t INV = 0xefffffffu;  // -r^-1 mod 2^32
};

template <class P>
struct Fp {
    uint32_t v[8];
};
using Fq = Fp<FqP>;
using Fr = Fp<FrP>;
struct Fq2 {
    Fq c0, c1;
};

template <class P>
BN_HD Fp<P> fp_zero() {
    Fp<P> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = 0;
    return r;
}
template <class P>
BN_HD Fp<P> fp_from(const uint32_t (&w)[8]) {
    Fp<P> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
}
// R mod q, R mod r (Montgomery one); R^2 (to convert into Montgomery form)
BN_HD Fq fq_one() { return fp_from<FqP>({0xc58f0d9du, 0xd35d438du, 0xf5c70b3du, 0x0a78eb28u, 0x7879462cu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}); }
BN_HD Fq fq_r2() { return fp_from<FqP>({0x538afa89u, 0xf32cfc5bu, 0xd44501fbu, 0xb5e71911u, 0x0a417ff6u, 0x47ab1effu, 0xcab8351fu, 0x06d89f71u}); }
BN_HD Fr fr_one() { return fp_from<FrP>({0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}); }
BN_HD Fr fr_r2() { return fp_from<FrP>({0xae216da7u, 0x1bb8e645u, 0xe35c59e3u, 0x53fe3ab1u, 0x53bb8085u, 0x8c49833du, 0x7f4e44a5u, 0x0216d0b1u}); }
// omega_{2^28} = 5^((r-1)/2^28) and its inverse, Montgomery form
BN_HD Fr fr_root28() { return fp_from<FrP>({0x80d13d9cu, 0x636e7355u, 0x2445ffd6u, 0xa22bf374u, 0x1eb203d8u, 0x56452ac0u, 0x2963f9e7u, 0x1860ef94u}); }
BN_HD Fr fr_root28_inv() { return fp_from<FrP>({0x584bb683u, 0x89bcc016u, 0x0164a50cu, 0xe8d9887fu, 0x795eda3du, 0x755e95cbu, 0x1323b130u, 0x0f572b87u}); }

template <class P>
BN_HD bool is_zero(const Fp<P>& a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= a.v[i];
    return o == 0;
}
template <class P>
BN_HD bool eq(const Fp<P>& a, const Fp<P>& b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i];
    return o == 0;
}
// a >= modulus (canonical-input check)
template <class P>
BN_HD bool ge_mod(const uint32_t* a) {
    for (int i = 7; i >= 0; i--) {
        if (a[i] != P::m(i)) return a[i] > P::m(i);
    }
    return true;
}

template <class P>
BN_HD Fp<P> add(const Fp<P>& a, const Fp<P>& b) {
    Fp<P> s, d;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)a.v[i] + b.v[i];
        s.v[i] = (uint32_t)c;
        c >>= 32;
    }
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        br += (int64_t)s.v[i] - P::m(i);
        d.v[i] = (uint32_t)br;
        br >>= 32;
    }
    // the moduli are below 2^254: a + b never carries out of 256 bits
    return br < 0 ? s : d;
}
template <class P>
BN_HD Fp<P> sub(const Fp<P>& a, const Fp<P>& b) {
    Fp<P> d, s;
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        br += (int64_t)a.v[i] - b.v[i];
        d.v[i] = (uint32_t)br;
        br >>= 32;
    }
    if (br == 0) return d;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)d.v[i] + P::m(i);
        s.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return s;
}
template <class P>
BN_HD Fp<P> neg(const Fp<P>& a) {
    return sub(fp_zero<P>(), a);
}
template <class P>
BN_HD Fp<P> dbl(const Fp<P>& a) {
    return add(a, a);
}

// CIOS Montgomery product a * b / 2^256 mod m
template <class P>
BN_HD Fp<P> mul(const Fp<P>& a, const Fp<P>& b) {
    uint32_t t[10];
#pragma unroll
    for (int i = 0; i < 10; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            uint64_t s = (uint64_t)a.v[j] * b.v[i] + t[j] + c;
            t[j] = (uint32_t)s;
            c = s >> 32;
        }
        uint64_t s = (uint64_t)t[8] + c;
        t[8] = (uint32_t)s;
        t[9] = (uint32_t)(s >> 32);
        uint32_t m = t[0] * P::INV;
        s = (uint64_t)m * P::m(0) + t[0];
        c = s >> 32;
#pragma unroll
        for (int j = 1; j < 8; j++) {
            s = (uint64_t)m * P::m(j) + t[j] + c;
            t[j - 1] = (uint32_t)s;
            c = s >> 32;
        }
        s = (uint64_t)t[8] + c;
        t[7] = (uint32_t)s;
        t[8] = t[9] + (uint32_t)(s >> 32);
    }
    Fp<P> r, d;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = t[i];
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        br += (int64_t)r.v[i] - P::m(i);
        d.v[i] = (uint32_t)br;
        br >>= 32;
    }
    return (br < 0 && t[8] == 0) ? r : d;
}
template <class P>
BN_HD Fp<P> sqr(const Fp<P>& a) {
    return mul(a, a);
}
template <class P>
BN_HD Fp<P> to_mont(const Fp<P>& a);
template <>
BN_HD Fq to_mont(const Fq& a) {
    return mul(a, fq_r2());
}
template <>
BN_HD Fr to_mont(const Fr& a) {
    return mul(a, fr_r2());
}
template <class P>
BN_HD Fp<P> from_mont(const Fp<P>& a) {
    Fp<P> one = fp_zero<P>();
    one.v[0] = 1;
    return mul(a, one);
}
// a^e for a little-endian 8-word exponent
template <class P>
BN_HD Fp<P> pow_words(const Fp<P>& a, const uint32_t* e, Fp<P> one) {
    Fp<P> r = one;
    for (int i = 255; i >= 0; i--) {
        r = sqr(r);
        if ((e[i >> 5] >> (i & 31)) & 1u) r = mul(r, a);
    }
    return r;
}
template <class P>
BN_HD Fp<P> pow_u64(const Fp<P>& a, uint64_t e, Fp<P> one) {
    Fp<P> r = one, b = a;
    while (e) {
        if (e & 1) r = mul(r, b);
        b = sqr(b);
        e >>= 1;
    }
    return r;
}
// Fermat inverse (0 -> 0)
BN_HD Fq inv(const Fq& a) {
    uint32_t e[8];
    for (int i = 0; i < 8; i++) e[i] = FqP::m(i);
    e[0] -= 2;  // q - 2 (no borrow: the low limb of q is odd and > 2)
    return pow_words(a, e, fq_one());
}
BN_HD Fr inv(const Fr& a) {
    uint32_t e[8];
    for (int i = 0; i < 8; i++) e[i] = FrP::m(i);
    e[0] -= 2;
    return pow_words(a, e, fr_one());
}

// ---- Fq2 ----
BN_HD bool is_zero(const Fq2& a) { return is_zero(a.c0) && is_zero(a.c1); }
BN_HD bool eq(const Fq2& a, const Fq2& b) { return eq(a.c0, b.c0) && eq(a.c1, b.c1); }
BN_HD Fq2 add(const Fq2& a, const Fq2& b) { return {add(a.c0, b.c0), add(a.c1, b.c1)}; }
BN_HD Fq2 sub(const Fq2& a, const Fq2& b) { return {sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
BN_HD Fq2 neg(const Fq2& a) { return {neg(a.c0), neg(a.c1)}; }
BN_HD Fq2 dbl(const Fq2& a) { return {dbl(a.c0), dbl(a.c1)}; }
BN_HD Fq2 mul(const Fq2& a, const Fq2& b) {
    Fq t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1);
    Fq t2 = mul(add(a.c0, a.c1), add(b.c0, b.c1));
    return {sub(t0, t1), sub(sub(t2, t0), t1)};
}
BN_HD Fq2 sqr(const Fq2& a) {
    Fq t = mul(a.c0, a.c1);
    return {mul(add(a.c0, a.c1), sub(a.c0, a.c1)), dbl(t)};
}
BN_HD Fq2 inv(const Fq2& a) {
    Fq d = inv(add(sqr(a.c0), sqr(a.c1)));
    return {mul(a.c0, d), neg(mul(a.c1, d))};
}
BN_HD Fq2 from_mont(const Fq2& a) { return {from_mont(a.c0), from_mont(a.c1)}; }
BN_HD Fq2 to_mont(const Fq2& a) { return {to_mont(a.c0), to_mont(a.c1)}; }

// curve coefficient b, Montgomery form: 3 on G1, 3/(9+u) on G2
BN_HD void curve_b(Fq& b) { b = fp_from<FqP>({0x50ad28d7u, 0x7a17caa9u, 0xe15521b9u, 0x1f6ac17au, 0x696bd284u, 0x334bea4eu, 0xce179d8eu, 0x2a1f6744u}); }
BN_HD void curve_b(Fq2& b) {
    b.c0 = fp_from<FqP>({0x77b802a8u, 0x3bf938e3u, 0x3633535du, 0x020b1b27u, 0x49755260u, 0x26b7edf0u, 0x4384a86du, 0x2514c632u});
    b.c1 = fp_from<FqP>({0xd1dcff67u, 0x38e7ecccu, 0x93ce0d3eu, 0x65f0b37du, 0x22ac00aau, 0xd749d0ddu, 0x4a688d4du, 0x0141b9ceu});
}
BN_HD void set_one(Fq& a) { a = fq_one(); }
BN_HD void set_one(Fq2& a) { a.c0 = fq_one(); a.c1 = fp_zero<FqP>(); }
BN_HD void set_zero(Fq& a) { a = fp_zero<FqP>(); }
BN_HD void set_zero(Fq2& a) { a.c0 = fp_zero<FqP>(); a.c1 = fp_zero<FqP>(); }

// ---- points ----
template <class F>
struct Aff {
    F x, y;
};
template <class F>
struct Xyzz {
    F x, y, zz, zzz;
};

template <class F>
BN_HD bool aff_is_inf(const Aff<F>& p) {
    return is_zero(p.x) && is_zero(p.y);
}
template <class F>
BN_HD bool on_curve(const Aff<F>& p) {
    if (aff_is_inf(p)) return true;
    F b;
    curve_b(b);
    return eq(sqr(p.y), add(mul(sqr(p.x), p.x), b));
}
template <class F>
BN_HD Xyzz<F> xyzz_inf() {
    Xyzz<F> r;
    set_one(r.x);
    set_one(r.y);
    set_zero(r.zz);
    set_zero(r.zzz);
    return r;
}
template <class F>
BN_HD bool is_inf(const Xyzz<F>& p) {
    return is_zero(p.zz);
}
template <class F>
BN_HD Xyzz<F> from_aff(const Aff<F>& a) {
    if (aff_is_inf(a)) return xyzz_inf<F>();
    Xyzz<F> r;
    r.x = a.x;
    r.y = a.y;
    set_one(r.zz);
    set_one(r.zzz);
    return r;
}
// dbl-2008-s-1 (a = 0)
template <class F>
BN_HD Xyzz<F> xyzz_dbl(const Xyzz<F>& p) {
    F u = dbl(p.y), v = sqr(u), w = mul(u, v), s = mul(p.x, v), x2 = sqr(p.x);
    F m = add(dbl(x2), x2);
    Xyzz<F> r;
    r.x = sub(sqr(m), dbl(s));
    r.y = sub(mul(m, sub(s, r.x)), mul(w, p.y));
    r.zz = mul(v, p.zz);
    r.zzz = mul(w, p.zzz);
    return r;  // ZZ = 0 stays 0: infinity (and a 2-torsion point) doubles to infinity
}
// mdbl-2008-s-1: double an affine point
template <class F>
BN_HD Xyzz<F> aff_dbl(const Aff<F>& p) {
    F u = dbl(p.y), v = sqr(u), w = mul(u, v), s = mul(p.x, v), x2 = sqr(p.x);
    F m = add(dbl(x2), x2);
    Xyzz<F> r;
    r.x = sub(sqr(m), dbl(s));
    r.y = sub(mul(m, sub(s, r.x)), mul(w, p.y));
    r.zz = v;
    r.zzz = w;
    return r;
}
// madd-2008-s: XYZZ + affine
template <class F>
BN_HD Xyzz<F> xyzz_add_aff(const Xyzz<F>& p, const Aff<F>& q) {
    if (aff_is_inf(q)) return p;
    if (is_inf(p)) return from_aff(q);
    F pp_ = sub(mul(q.x, p.zz), p.x);
    F rr = sub(mul(q.y, p.zzz), p.y);
    if (is_zero(pp_)) {
        if (is_zero(rr)) return aff_dbl(q);
        return xyzz_inf<F>();
    }
    F pp = sqr(pp_), ppp = mul(pp_, pp), qq = mul(p.x, pp);
    Xyzz<F> r;
    r.x = sub(sub(sqr(rr), ppp), dbl(qq));
    r.y = sub(mul(rr, sub(qq, r.x)), mul(p.y, ppp));
    r.zz = mul(p.zz, pp);
    r.zzz = mul(p.zzz, ppp);
    return r;
}
// add-2008-s: XYZZ + XYZZ
template <class F>
BN_HD Xyzz<F> xyzz_add(const Xyzz<F>& p, const Xyzz<F>& q) {
    if (is_inf(q)) return p;
    if (is_inf(p)) return q;
    F u1 = mul(p.x, q.zz), u2 = mul(q.x, p.zz);
    F s1 = mul(p.y, q.zzz), s2 = mul(q.y, p.zzz);
    F pp_ = sub(u2, u1), rr = sub(s2, s1);
    if (is_zero(pp_)) {
        if (is_zero(rr)) return xyzz_dbl(p);
        return xyzz_inf<F>();
    }
    F pp = sqr(pp_), ppp = mul(pp_, pp), qq = mul(u1, pp);
    Xyzz<F> r;
    r.x = sub(sub(sqr(rr), ppp), dbl(qq));
    r.y = sub(mul(rr, sub(qq, r.x)), mul(s1, ppp));
    r.zz = mul(mul(p.zz, q.zz), pp);
    r.zzz = mul(mul(p.zzz, q.zzz), ppp);
    return r;
}
// k * p for a small k (k < 2^32)
template <class F>
BN_HD Xyzz<F> xyzz_mul_small(const Xyzz<F>& p, uint32_t k) {
    Xyzz<F> r = xyzz_inf<F>();
    if (k == 0) return r;
    for (int i = 31 - __builtin_clz(k); i >= 0; i--) {
        r = xyzz_dbl(r);
        if ((k >> i) & 1u) r = xyzz_add(r, p);
    }
    return r;
}
// affine, canonical (not Montgomery) coordinates; infinity -> zeros
template <class F>
BN_HD Aff<F> to_affine_canonical(const Xyzz<F>& p) {
    Aff<F> r;
    if (is_inf(p)) {
        set_zero(r.x);
        set_zero(r.y);
        return r;
    }
    r.x = from_mont(mul(p.x, inv(p.zz)));
    r.y = from_mont(mul(p.y, inv(p.zzz)));
    return r;
}

}  // namespace bn
