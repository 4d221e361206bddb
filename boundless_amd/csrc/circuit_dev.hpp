// circuit_dev.hpp — the arithmetic core shared by witness generation and eval_check: the value of one derived cell,
//     sum_{t<T} prod_{f<G} pool[idx(t,f)]            (include/bx_prover.h, "The synthetic circuit")
// Both knobs are compile-time for the shapes the prover is tuned for (every pool reference is then a fixed register);
// <0, 0> is the run-time fallback for any other (T, G) and uses plain canonical arithmetic.
//
// The compile-time paths run on the signed, bounded Montgomery arithmetic of poseidon2_arith.hpp (sredc(t) = (t + mP)/2^32,
// |result| <= ub(|t|) = |t|/2^32 + P/2 + 1, valid for |t| <= SREDC_MAX = 1.209 P^2; P^2/2^32 = 0.469 P) so that no product is
// followed by a conditional subtraction and the sums stay unreduced in 64 bits.  Pool entries are centred once per cell, |c| <= P/2.
//
// G >= 3, the factored form.  pool_idx(t, 0) runs through all 16 pool entries on every block of 16 terms, so entry a is the first
// factor of T/16 terms and   sum_{t: idx(t,0)=a} pool[a] * (rest of t)  =  pool[a] * sum_t (rest of t):  the product with pool[a]
// is taken once per group of terms instead of once per term (one reduced product, 3 multiply-class instructions, less per term;
// one reduction and one multiply-add more per group).  Every step is a congruence mod P and every path from a term to the result
// passes G - 1 + 2 reductions against two factors R, as in the term-by-term form, so the canonical result is the same word.
//   the rest of a term    y = pool[idx(t,1)],  y <- sredc(y * pool[idx(t,f)]) for f = 2 .. G-2,  then  y * pool[idx(t,G-1)]:
//                         G = 3: |y| <= 0.5 P, term <= 0.25 P^2;   G = 4: |y| <= 0.617 P, term <= 0.309 P^2;
//                         G >= 5: |y| <= 0.65 P for any chain length, term <= 0.325 P^2
//   inner group           inner = sum of <= ISZ terms with the same first factor:  G = 3: ISZ = 4, |inner| <= 1.0 P^2;
//                         G >= 4: ISZ = 3 (four terms would be 1.234 P^2 > SREDC_MAX).  An entry with more terms than ISZ gets
//                         several inner groups of balanced size (four terms at G = 4: 2 + 2, |inner| <= 0.617 P^2)
//   its reduction         s = sredc(inner):   G = 3: |s| <= 0.97 P (4 terms), 0.85 P (3);   G = 4: 0.79 P (2 terms), 0.93 P (3)
//   outer group           outer = sum of s * pool[a] over consecutive inner groups, as many as keep it <= SREDC_MAX:
//                         G = 3: 2 groups of 4 terms (0.97 P^2);   G = 4: 3 groups of 2 terms (1.18 P^2), 2 groups of 3 (0.93 P^2)
//   its reduction         r = sredc(outer):   |r| <= 1.06 P at most (G = 4, T = 64), still an int32
//   second level          acc2 = sum of r * R over consecutive outer groups  (R = 2^32 mod P = 0.1334 P, so sredc(acc2) == sum r),
//                         as many as keep |acc2| <= FINAL_MAX = 1.0667 P^2, the largest operand whose reduction is < P in magnitude
//   third level           the same over the second-level results (one group; more is refused at compile time)
// ConsPlan builds the groups at compile time from pool_idx and carries the bound of every accumulator with them; cons_sum's
// static_asserts hold the plan to SREDC_MAX / FINAL_MAX, and the host build (BX_CHECK_BOUNDS) asserts every sredc operand it meets.
//
// G <= 2 has no shared product to factor out and keeps the term-by-term form:
//   a group of 3 terms        acc = sum x * c_last:         |acc| <= 3 * 0.5 P * 0.5 P = 0.75 P^2
//   its reduction             r = sredc(acc):               |r| <= 0.85 P
//   second level, 8 groups    acc2 = sum r * R:             |acc2| <= 8 * 0.85 * 0.1334 P^2 = 0.91 P^2,  |r2| <= 0.93 P
//   third level, <= 7 second-level results, same form:      |acc3| <= 7 * 0.93 * 0.1334 P^2 = 0.87 P^2,  |r3| <= 0.91 P
// In both forms the last reduction is < P in magnitude, so one conditional add of P makes it canonical, and the result is
// bit-identical to the plain form; tests compare both paths with the oracle.
#pragma once
#include "circuit.hpp"
#include "fp.hpp"
#include "poseidon2_arith.hpp"

namespace bx {
inline namespace BX_MAD_FLAVOUR {

// largest sredc operand whose result is < P in magnitude: ub(FINAL_MAX) = P - 1
constexpr i64 FINAL_MAX = ((i64)(P / 2) - 1) * ((i64)1 << 32);
static_assert(ub(FINAL_MAX) < (i64)P && FINAL_MAX <= SREDC_MAX, "FINAL_MAX");

// f(IntC<I>{}) for I = BEGIN .. END-1, unrolled at compile time: the counter reaches the body as a constant expression
template <int V>
struct IntC {
    static constexpr int value = V;
};
template <int BEGIN, int END, class F>
BX_HD void static_for(F&& f) {
    if constexpr (BEGIN < END) {
        f(IntC<BEGIN>{});
        static_for<BEGIN + 1, END>(f);
    }
}

// The grouping of the factored form for one (T, G), with the magnitude bound of every accumulator (all pool entries at +-P/2).
template <int TT, int GG>
struct ConsPlan {
    static constexpr int NPOOL = (int)Circuit::POOL;
    static constexpr i64 BC = (i64)(P / 2);                   // a centred pool entry
    static constexpr i64 chain_bound() {                      // y before its last product
        i64 y = BC;
        for (int f = 2; f + 1 < GG; ++f) y = ub(y * BC);
        return y;
    }
    static constexpr i64 TERM = chain_bound() * BC;           // one term of an inner accumulator
    static constexpr int ISZ = (int)(SREDC_MAX / TERM) < 4 ? (int)(SREDC_MAX / TERM) : 4;  // terms per inner group, at most
    static_assert(ISZ >= 1 && ISZ * TERM <= SREDC_MAX, "cons_sum: inner group beyond sredc's range");

    int nq = 0, no = 0, n2 = 0;            // inner groups, outer groups, second-level groups
    int first[TT]{}, len[TT]{}, term[TT][ISZ]{};  // inner group q: its shared first factor, its terms
    int obeg[TT + 1]{}, lbeg[TT + 1]{};    // outer group o = inner groups [obeg[o], obeg[o+1]), second-level group l likewise
    i64 max_inner = 0, max_outer = 0, max_l2 = 0, max_l3 = 0;

    constexpr ConsPlan() {
        // inner groups in the order (g, a): the g-th group of every pool entry before any (g+1)-th, so that an outer group never
        // holds two groups of one entry (hipcc would add their reductions first and emulate a 64 x 32-bit product for the sum)
        for (int g = 0; g < TT; ++g)
            for (int a = 0; a < NPOOL; ++a) {
                int members[TT]{}, n = 0;
                for (int t = 0; t < TT; ++t)
                    if ((int)Circuit::pool_idx((unsigned)t, 0u) == a) members[n++] = t;
                const int groups = (n + ISZ - 1) / ISZ;
                if (g >= groups) continue;
                // balanced: sizes differ by at most one
                const int sz = n / groups + (g < n % groups ? 1 : 0), at = g * (n / groups) + (g < n % groups ? g : n % groups);
                first[nq] = a;
                len[nq] = sz;
                for (int k = 0; k < sz; ++k) term[nq][k] = members[at + k];
                if (sz * TERM > max_inner) max_inner = sz * TERM;
                ++nq;
            }
        i64 rb[TT + 1]{};                  // bound of each outer group's reduction
        i64 cur = 0;
        for (int q = 0; q < nq; ++q) {     // outer groups: consecutive inner groups while the sum stays reducible
            const i64 add = ub(len[q] * TERM) * BC;
            if (q > 0 && cur + add > SREDC_MAX) {
                rb[no++] = ub(cur);
                obeg[no] = q;
                cur = 0;
            }
            cur += add;
            if (cur > max_outer) max_outer = cur;
        }
        rb[no++] = ub(cur);
        obeg[no] = nq;
        cur = 0;
        for (int o = 0; o < no; ++o) {     // second level: consecutive outer groups while the reduction stays below P
            const i64 add = rb[o] * (i64)MONT_ONE;
            if (o > 0 && cur + add > FINAL_MAX) {
                max_l3 += ub(cur) * (i64)MONT_ONE;
                lbeg[++n2] = o;
                cur = 0;
            }
            cur += add;
            if (cur > max_l2) max_l2 = cur;
        }
        max_l3 += ub(cur) * (i64)MONT_ONE;
        lbeg[++n2] = no;
    }
};
template <int TT, int GG>
inline constexpr ConsPlan<TT, GG> cons_plan{};

template <int TT, int GG>
BX_HD uint32_t cons_sum(const uint32_t (&pool_u)[Circuit::POOL], uint32_t T, uint32_t G) {
    if constexpr (TT > 0 && GG >= 3) {
        constexpr int N2 = cons_plan<TT, GG>.n2;
        static_assert(cons_plan<TT, GG>.max_inner <= SREDC_MAX && cons_plan<TT, GG>.max_outer <= SREDC_MAX, "cons_sum: a group sum beyond sredc's range");
        static_assert(cons_plan<TT, GG>.max_l2 <= FINAL_MAX && cons_plan<TT, GG>.max_l3 <= FINAL_MAX, "cons_sum: term count beyond the three reduction levels");
        i32 pool[Circuit::POOL];
#pragma unroll
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = fp_centre(pool_u[i]);
        // every index below is a constant expression (static_for hands its counter over as a type), so each pool reference is a
        // fixed register and each accumulator a fresh value of its group
        i64 acc3 = 0;
        i32 result = 0;
        static_for<0, N2>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            i64 acc2 = 0;
            static_for<cons_plan<TT, GG>.lbeg[l], cons_plan<TT, GG>.lbeg[l + 1]>([&](auto oc) {
                constexpr int o = decltype(oc)::value;
                i64 outer = 0;
                static_for<cons_plan<TT, GG>.obeg[o], cons_plan<TT, GG>.obeg[o + 1]>([&](auto qc) {
                    constexpr int q = decltype(qc)::value;
                    i64 inner = 0;
                    static_for<0, cons_plan<TT, GG>.len[q]>([&](auto kc) {
                        constexpr int k = decltype(kc)::value;
                        constexpr unsigned t = (unsigned)cons_plan<TT, GG>.term[q][k];
                        i32 y = pool[Circuit::pool_idx(t, 1u)];
#pragma unroll
                        for (int f = 2; f + 1 < GG; ++f) y = sredc(smul(y, pool[Circuit::pool_idx(t, (unsigned)f)], f), f);
                        inner = smad(y, pool[Circuit::pool_idx(t, (unsigned)(GG - 1))], inner, k);
                    });
                    outer = smad(sredc(inner, 3), pool[cons_plan<TT, GG>.first[q]], outer, q);
                });
                acc2 = smad_k(sredc(outer, 1), MONT_ONE, acc2, o);
            });
            const i32 r2 = sredc(acc2, 2);
            if constexpr (N2 == 1) result = r2;
            else acc3 = smad_k(r2, MONT_ONE, acc3, l);
        });
        if constexpr (N2 > 1) result = sredc(acc3, 0);
        return (uint32_t)(result + (result < 0 ? (i32)P : 0));
    } else if constexpr (TT > 0) {
        static_assert(TT <= 3 * 8 * 7 && GG >= 1, "cons_sum: term count beyond the three reduction levels");
        i32 pool[Circuit::POOL];
#pragma unroll
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = fp_centre(pool_u[i]);
        constexpr int GRP = 3, NG = (TT + GRP - 1) / GRP;
        i64 acc2 = 0, acc3 = 0;
        i32 result = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int nk = (g + 1) * GRP <= TT ? GRP : TT - g * GRP;
            i64 acc = 0;
#pragma unroll
            for (int k = 0; k < GRP; ++k) {
                if (k < nk) {
                    const i32 x = pool[Circuit::pool_idx((unsigned)(g * GRP + k), 0u)];
                    if constexpr (GG == 1) acc = smad_k(x, MONT_ONE, acc, k);
                    else acc = smad(x, pool[Circuit::pool_idx((unsigned)(g * GRP + k), 1u)], acc, k);
                }
            }
            const i32 r = sredc(acc, 3);
            acc2 = smad_k(r, MONT_ONE, acc2, g);
            if ((g & 7) == 7 || g == NG - 1) {
                const i32 r2 = sredc(acc2, 1);
                acc2 = 0;
                if constexpr (NG <= 8) result = r2;
                else acc3 = smad_k(r2, MONT_ONE, acc3, 2);
            }
        }
        if constexpr (NG > 8) result = sredc(acc3, 0);
        return (uint32_t)(result + (result < 0 ? (i32)P : 0));
    } else {
        uint32_t sum = 0;
        for (uint32_t t = 0; t < T; ++t) {
            uint32_t prod = pool_u[Circuit::pool_idx(t, 0u)];
            for (uint32_t f = 1; f < G; ++f) prod = fp_mul(prod, pool_u[Circuit::pool_idx(t, f)]);
            sum = fp_add(sum, prod);
        }
        return sum;
    }
}

// The walk over the derived columns j = 0 .. J-1 that witness generation (one thread per row) and eval_check (one thread per domain
// point) share keeps the pool of column F+j in registers from one column to the next: the eight previous derived columns in `ring`
// (csel(0..7) before the first), free columns j, j+1, j+2 in `u`, code csel(j..j+3) in `k`.  Slot 1 alone is loaded per column,
// where Circuit::slot1_back asks for a row back (else it repeats slot 0).  Circuit::pool_src states the same rule for the host.
struct DerivedRegs {
    uint32_t ring[8], u[3], k[4];
    // the pool of the column the walk stands at
    BX_HD void fill(uint32_t (&pool)[Circuit::POOL], uint32_t slot1) const {
        pool[0] = u[0]; pool[1] = slot1; pool[2] = u[1]; pool[3] = u[2];
#pragma unroll
        for (int q = 0; q < 8; ++q) pool[4 + q] = ring[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) pool[12 + q] = k[q];
    }
    // on to column j+1: d = the value of column F+j, next_u = free column (j+3) mod F, next_k = code csel(j+4)
    BX_HD void shift(uint32_t d, uint32_t next_u, uint32_t next_k) {
#pragma unroll
        for (int q = 7; q > 0; --q) ring[q] = ring[q - 1];
        ring[0] = d;
        u[0] = u[1]; u[1] = u[2]; u[2] = next_u;
        k[0] = k[1]; k[1] = k[2]; k[2] = k[3]; k[3] = next_k;
    }
};

}  // inline namespace BX_MAD_FLAVOUR
}  // namespace bx
