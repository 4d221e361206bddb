// circuit_dev.hpp — the arithmetic core shared by witness generation and eval_check: the value of one derived cell,
//     sum_{t<T} prod_{f<G} pool[idx(t,f)]            (include/bx_prover.h, "The synthetic circuit")
// Both knobs are compile-time for the shapes the prover is tuned for (every pool reference is then a fixed register);
// <0, 0> is the run-time fallback for any other (T, G) and uses plain canonical arithmetic.
//
// The compile-time paths run on the signed, bounded Montgomery arithmetic of poseidon2_arith.hpp (sredc(t) = (t + mP)/2^32,
// |result| <= ub(|t|) = |t|/2^32 + P/2 + 1, valid for |t| <= SREDC_MAX = 1.209 P^2; P^2/2^32 = 0.469 P) so that no product is
// followed by a conditional subtraction and the sums stay unreduced in 64 bits.  Pool entries are centred, |c| <= P/2: by the walk of
// circuit.hip once per word, where it enters the registers (DerivedRegs<true> and the centred entry of cons_sum, 4 of the 16 entries
// are new per cell), by the canonical-pool signature once per call.  The second and third level multiply by an opaque copy of R
// (smad_r) so that each addend stays one v_mad_i64_i32.  Compiled, the walk's loop body per cell, VALU instructions / multiplies
// (v_mad_i64_i32 + v_mul_lo_u32 + v_mad_u64_u32): witness_derive_kernel<64,4> 412 / 251 -> 312 / 274 (54 VGPRs, it was 65),
// eval_check_kernel<64,4> 467 / 275 -> 367 / 298 (78 VGPRs, it was 87: six waves per SIMD again).  The multiplies that came are the
// level steps that had been folded into emulated 64 x 32-bit products; the 123 other instructions that went are that emulation's sign
// extensions, 64-bit adds and copies, and the centring of twelve entries that had been centred a cell before.
//
// G = 4, the pair form.  A term is a product of four pool entries and can be written as (pair) * (pair) in three ways; PairPlan picks
// one split per term so that pairs recur (44 distinct pairs serve the 128 pair slots of T = 64, where the first-factor form below
// computes 59 reduced products and 64 + 32 multiply-adds), and a term is then ONE multiply-add of two shared, reduced pair products.
// The plan: each term's most popular split, four sweeps that re-choose a term's split where that frees a pair (51 pairs), then two
// passes that drop a little-used pair outright by moving all its users to other splits (44).
//   a pair                p = sredc(c_a * c_b), computed at its first use:   |p| <= ub(P^2/4) = 0.617 P
//   a group               acc = sum of <= GRP = 3 terms p1 * p2:             |acc| <= 3 * 0.381 P^2 = 1.143 P^2 <= SREDC_MAX (four: 1.52)
//                         no two terms of a group share a pair: hipcc would rewrite p*q1 + p*q2 as p*(q1 + q2) with a 64-bit sum
//                         and emulate a 64 x 32-bit product
//   its reduction         r = sredc(acc):                                    |r| <= 1.036 P, still an int32
//   second level          acc2 = sum of r * R over <= 7 consecutive groups:  |acc2| <= 0.967 P^2 <= FINAL_MAX (eight: 1.105 P^2)
//   third level           the same over the <= 4 second-level results:       |acc3| <= 4 * (P - 1) * R = 0.53 P^2
// The terms are ordered so that a pair's uses lie in neighbouring groups (at most 7 pairs are computed and still awaited at any
// point of T = 64), which keeps the pair products from costing registers: eval_check_kernel<64,4> compiles to 78 VGPRs, no scratch.
// Every path from a term to the result is again a congruence mod P through three reductions against two factors R, so the
// canonical result is the same word as the first-factor form's and the plain loop's.  PairPlan carries the bounds; cons_sum's
// static_asserts hold them, and the host build (BX_CHECK_BOUNDS) asserts every pair, every sredc operand and every level's sum.
//
// G = 3 and G >= 5, the factored form (ConsPlan; built for G = 4 too, where tests read it, but no longer executed there).
// pool_idx(t, 0) runs through all 16 pool entries on every block of 16 terms, so entry a is the first factor of T/16 terms
// and   sum_{t: idx(t,0)=a} pool[a] * (rest of t)  =  pool[a] * sum_t (rest of t):  the product with pool[a]
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
#include <type_traits>

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

// The plan of the pair form (G = 4) for one T: which of its three splits into two pairs each term takes, the distinct pairs in
// the order of their first use, and the terms in the order they are summed, cut into groups, with the bound of every accumulator.
template <int TT>
struct PairPlan {
    static constexpr int NPOOL = (int)Circuit::POOL, NID = NPOOL * NPOOL;
    static constexpr i64 BC = (i64)(P / 2);                   // a centred pool entry
    static constexpr i64 PAIR = ub(BC * BC);                  // a reduced pair product
    static constexpr i64 TERM = PAIR * PAIR;                  // one term of a group
    static constexpr int GRP = (int)(SREDC_MAX / TERM);       // terms per group, at most
    static_assert(GRP == 3 && GRP * TERM <= SREDC_MAX, "cons_sum: pair group beyond sredc's range");
    static constexpr int pair_id(unsigned a, unsigned b) { return a < b ? (int)(a * NPOOL + b) : (int)(b * NPOOL + a); }

    int np = 0, ng = 0, n2 = 0;            // distinct pairs, groups, second-level groups
    int pa[2 * TT]{}, pb[2 * TT]{};        // pair p = pool[pa[p]] * pool[pb[p]], numbered by first use
    int seq[TT]{}, s1[TT]{}, s2[TT]{};     // slot s sums term seq[s] = pair s1[s] * pair s2[s]
    int pbeg[TT + 1]{};                    // pairs [pbeg[s], pbeg[s+1]) are computed at slot s, their first use
    int gbeg[TT + 1]{}, lbeg[TT + 1]{};    // group g = slots [gbeg[g], gbeg[g+1]), second-level group l = groups [lbeg[l], lbeg[l+1])
    int max_live = 0;                      // most pairs computed and still to be used at any slot
    i64 max_group = 0, max_l2 = 0, max_l3 = 0;

    constexpr PairPlan() {
        // the three splits of every term: factor 0 with factor s+1, and the other two
        int sp[TT][3][2]{}, pop[NID]{}, ref[NID]{}, ch[TT]{};
        for (int t = 0; t < TT; ++t) {
            unsigned x[4]{};
            for (unsigned f = 0; f < 4; ++f) x[f] = Circuit::pool_idx((unsigned)t, f);
            for (int s = 0; s < 3; ++s) {
                sp[t][s][0] = pair_id(x[0], x[s + 1]);
                sp[t][s][1] = pair_id(x[s == 0 ? 2 : 1], x[s == 2 ? 2 : 3]);
                ++pop[sp[t][s][0]];
                ++pop[sp[t][s][1]];
            }
        }
        // start from each term's most popular split, then re-choose a term's split where that frees a pair; ref[] counts the
        // uses of every pair under the current choice and is kept up to date, so a trial costs three look-ups
        for (int t = 0; t < TT; ++t) {
            for (int s = 1; s < 3; ++s)
                if (pop[sp[t][s][0]] + pop[sp[t][s][1]] > pop[sp[t][ch[t]][0]] + pop[sp[t][ch[t]][1]]) ch[t] = s;
            ++ref[sp[t][ch[t]][0]];
            ++ref[sp[t][ch[t]][1]];
        }
        for (int sweep = 0; sweep < 4; ++sweep)
            for (int t = 0; t < TT; ++t) {
                --ref[sp[t][ch[t]][0]];
                --ref[sp[t][ch[t]][1]];
                int best = 0, best_new = 3, best_ref = 0;
                for (int s = 0; s < 3; ++s) {
                    const int a = sp[t][s][0], b = sp[t][s][1];
                    const int fresh = (ref[a] == 0) + (ref[b] == 0 && b != a), shared = ref[a] + ref[b];
                    if (fresh < best_new || (fresh == best_new && shared > best_ref)) best = s, best_new = fresh, best_ref = shared;
                }
                ch[t] = best;
                ++ref[sp[t][best][0]];
                ++ref[sp[t][best][1]];
            }
        // then pairs with few uses are dropped outright: all users of pair p move to splits without it, and the move stays if fewer
        // distinct pairs remain — in the second pass also if as many, a sideways step after which further pairs can go.  Pairs are
        // tried by rising use count; `delta` follows the distinct count through ref[], so a trial never rescans the terms' pairs.
        for (int pass = 0; pass < 2; ++pass) {
            int snap[NID]{};
            for (int i = 0; i < NID; ++i) snap[i] = ref[i];
            for (int r = 1; r <= 4; ++r)
                for (int p = 0; p < NID; ++p) {
                    if (snap[p] != r || ref[p] == 0 || ref[p] > 4) continue;
                    int users[4]{}, was[4]{}, nu = 0, moved = 0, delta = 0;
                    for (int t = 0; t < TT; ++t)
                        if (sp[t][ch[t]][0] == p || sp[t][ch[t]][1] == p) users[nu++] = t;
                    for (int u = 0; u < nu; ++u) {
                        was[u] = ch[users[u]];
                        for (int k = 0; k < 2; ++k) delta -= (--ref[sp[users[u]][was[u]][k]] == 0);
                    }
                    for (; moved < nu; ++moved) {
                        const int t = users[moved];
                        int best = -1, best_new = 3, best_ref = 0;
                        for (int s = 0; s < 3; ++s) {
                            const int a = sp[t][s][0], b = sp[t][s][1];
                            if (a == p || b == p) continue;
                            const int fresh = (ref[a] == 0) + (ref[b] == 0 && b != a), shared = ref[a] + ref[b];
                            if (best < 0 || fresh < best_new || (fresh == best_new && shared > best_ref)) best = s, best_new = fresh, best_ref = shared;
                        }
                        if (best < 0) break;   // every split of this term holds p
                        ch[t] = best;
                        for (int k = 0; k < 2; ++k) delta += (ref[sp[t][best][k]]++ == 0);
                    }
                    if (moved < nu || delta > 0 || (delta == 0 && pass == 0)) {   // not better: put everything back
                        for (int u = 0; u < moved; ++u)
                            for (int k = 0; k < 2; ++k) --ref[sp[users[u]][ch[users[u]]][k]];
                        for (int u = 0; u < nu; ++u) {
                            ch[users[u]] = was[u];
                            for (int k = 0; k < 2; ++k) ++ref[sp[users[u]][was[u]][k]];
                        }
                    }
                }
        }
        // the order: the next term is the one that needs the fewest pairs not yet computed, then the one that uses the most pairs
        // for the last time, so that a pair's uses lie close together.  No two terms of a group share a pair (hipcc would rewrite
        // p*q1 + p*q2 as p*(q1 + q2) with a 64-bit sum and emulate a 64 x 32-bit product), so such terms go to neighbouring groups.
        int num[NID]{}, live = 0, glen = 0, gp[2 * GRP]{};
        bool placed[TT]{};
        for (int i = 0; i < NID; ++i) num[i] = -1;
        for (int slot = 0; slot < TT;) {
            int best = -1, best_new = 3, best_last = -1;
            if (glen < GRP)
                for (int t = 0; t < TT; ++t) {
                    if (placed[t]) continue;
                    const int a = sp[t][ch[t]][0], b = sp[t][ch[t]][1];
                    bool clash = false;
                    for (int k = 0; k < 2 * glen; ++k) clash = clash || gp[k] == a || gp[k] == b;
                    if (clash) continue;
                    const int fresh = (num[a] < 0) + (num[b] < 0 && b != a);
                    const int last = a == b ? (ref[a] == 2) : (ref[a] == 1) + (ref[b] == 1);
                    if (fresh < best_new || (fresh == best_new && last > best_last)) best = t, best_new = fresh, best_last = last;
                }
            if (best < 0) {                // the group is full, or every term left shares a pair with it
                gbeg[++ng] = slot;
                glen = 0;
                continue;
            }
            const int a = sp[best][ch[best]][0], b = sp[best][ch[best]][1];
            for (int k = 0; k < 2; ++k) {
                const int id = k ? b : a;
                if (num[id] < 0) {
                    num[id] = np;
                    pa[np] = id / NPOOL;
                    pb[np] = id % NPOOL;
                    ++np;
                    ++live;
                }
            }
            if (live > max_live) max_live = live;
            live -= (--ref[a] == 0);
            live -= (--ref[b] == 0);
            placed[best] = true;
            seq[slot] = best;
            s1[slot] = num[a];
            s2[slot] = num[b];
            gp[2 * glen] = a;
            gp[2 * glen + 1] = b;
            ++glen;
            pbeg[++slot] = np;
        }
        gbeg[++ng] = TT;
        i64 cur = 0;
        for (int g = 0; g < ng; ++g) {     // second level: consecutive groups while the reduction stays below P
            const i64 sum = (gbeg[g + 1] - gbeg[g]) * TERM, add = ub(sum) * (i64)MONT_ONE;
            if (sum > max_group) max_group = sum;
            if (g > 0 && cur + add > FINAL_MAX) {
                max_l3 += ub(cur) * (i64)MONT_ONE;
                lbeg[++n2] = g;
                cur = 0;
            }
            cur += add;
            if (cur > max_l2) max_l2 = cur;
        }
        max_l3 += ub(cur) * (i64)MONT_ONE;
        lbeg[++n2] = ng;
    }
};
template <int TT>
inline constexpr PairPlan<TT> pair_plan{};

// r * R + c, the step of the second and third reduction level.  In a translation unit that leaves its multiply-adds to the compiler
// (BX_PLAIN_MAD) the device build multiplies by an opaque copy of R, one per use: with the constant in sight hipcc rewrites a level's
// sum of r_i * R as (sum of r_i) * R, sign-extends every r_i, adds them in 64 bits and emulates a 64 x 32-bit product (about 28
// instructions for a level of seven, where this is 7 v_mad_i64_i32).  The copy lives in an SGPR (an s_mov per use, no VALU work), is
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

// The compile-time paths, on a pool that is already centred: |pool[i]| <= P/2 is what every bound of the plans rests on, and the
// host build (BX_CHECK_BOUNDS) asserts it for every entry.  The walk of circuit.hip calls this with the pool its DerivedRegs<true>
// keep centred from cell to cell; the canonical-pool signature below centres and forwards.
template <int TT, int GG>
BX_HD uint32_t cons_sum(const i32 (&pool)[Circuit::POOL], uint32_t /*T*/, uint32_t /*G*/) {
    static_assert(TT > 0 && GG > 0, "cons_sum: the run-time form takes a canonical pool");
#pragma unroll
    for (unsigned i = 0; i < Circuit::POOL; ++i) BX_ASSERT_BOUND(pool[i] <= (i32)(P / 2) && pool[i] >= -(i32)(P / 2), "cons_sum: a pool entry that is not centred");
    if constexpr (GG == 4) {
        constexpr int N2 = pair_plan<TT>.n2;
        static_assert(pair_plan<TT>.max_group <= SREDC_MAX, "cons_sum: a group sum beyond sredc's range");
        static_assert(pair_plan<TT>.max_l2 <= FINAL_MAX && pair_plan<TT>.max_l3 <= FINAL_MAX, "cons_sum: term count beyond the three reduction levels");
        // every index below is a constant expression, so each pool entry and each pair product is a fixed register
        i32 pr[pair_plan<TT>.np];
        i64 acc3 = 0;
        i32 result = 0;
        static_for<0, N2>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            i64 acc2 = 0;
            static_for<pair_plan<TT>.lbeg[l], pair_plan<TT>.lbeg[l + 1]>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                i64 acc = 0;
                static_for<pair_plan<TT>.gbeg[g], pair_plan<TT>.gbeg[g + 1]>([&](auto sc) {
                    constexpr int s = decltype(sc)::value;
                    static_for<pair_plan<TT>.pbeg[s], pair_plan<TT>.pbeg[s + 1]>([&](auto pc) {
                        constexpr int p = decltype(pc)::value;
                        pr[p] = sredc(smul(pool[pair_plan<TT>.pa[p]], pool[pair_plan<TT>.pb[p]], p), p);
                        BX_ASSERT_BOUND(pr[p] <= PairPlan<TT>::PAIR && pr[p] >= -PairPlan<TT>::PAIR, "cons_sum pair");
                    });
                    acc = smad(pr[pair_plan<TT>.s1[s]], pr[pair_plan<TT>.s2[s]], acc, s);
                });
                acc2 = smad_r(sredc(acc, 3), acc2, g);
            });
            BX_ASSERT_BOUND(acc2 <= FINAL_MAX && acc2 >= -FINAL_MAX, "cons_sum second level");
            const i32 r2 = sredc(acc2, 2);
            if constexpr (N2 == 1) result = r2;
            else acc3 = smad_r(r2, acc3, l);
        });
        if constexpr (N2 > 1) {
            BX_ASSERT_BOUND(acc3 <= FINAL_MAX && acc3 >= -FINAL_MAX, "cons_sum third level");
            result = sredc(acc3, 0);
        }
        return (uint32_t)(result + (result < 0 ? (i32)P : 0));
    } else if constexpr (GG >= 3) {
        constexpr int N2 = cons_plan<TT, GG>.n2;
        static_assert(cons_plan<TT, GG>.max_inner <= SREDC_MAX && cons_plan<TT, GG>.max_outer <= SREDC_MAX, "cons_sum: a group sum beyond sredc's range");
        static_assert(cons_plan<TT, GG>.max_l2 <= FINAL_MAX && cons_plan<TT, GG>.max_l3 <= FINAL_MAX, "cons_sum: term count beyond the three reduction levels");
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
                acc2 = smad_r(sredc(outer, 1), acc2, o);
            });
            const i32 r2 = sredc(acc2, 2);
            if constexpr (N2 == 1) result = r2;
            else acc3 = smad_r(r2, acc3, l);
        });
        if constexpr (N2 > 1) result = sredc(acc3, 0);
        return (uint32_t)(result + (result < 0 ? (i32)P : 0));
    } else {
        static_assert(TT <= 3 * 8 * 7 && GG >= 1, "cons_sum: term count beyond the three reduction levels");
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
            acc2 = smad_r(r, acc2, g);
            if ((g & 7) == 7 || g == NG - 1) {
                const i32 r2 = sredc(acc2, 1);
                acc2 = 0;
                if constexpr (NG <= 8) result = r2;
                else acc3 = smad_r(r2, acc3, 2);
            }
        }
        if constexpr (NG > 8) result = sredc(acc3, 0);
        return (uint32_t)(result + (result < 0 ? (i32)P : 0));
    }
}

// The canonical-pool signature: the compile-time paths centre the pool and take the entry above; <0, 0> is the run-time form on
// canonical words.
template <int TT, int GG>
BX_HD uint32_t cons_sum(const uint32_t (&pool_u)[Circuit::POOL], uint32_t T, uint32_t G) {
    if constexpr (TT > 0) {
        i32 pool[Circuit::POOL];
#pragma unroll
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = fp_centre(pool_u[i]);
        return cons_sum<TT, GG>(pool, T, G);
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
// CENTRED (the compile-time paths of cons_sum): the registers hold centred words, |c| <= P/2.  A word is centred once, by enter(),
// where it is loaded or produced — the 8 + 3 + 4 initial loads, slot 1's back-tap, and per column the derived value, the next free
// column and the next code selector — where centring the whole pool per cell redid twelve of sixteen entries.  Only the registers
// are centred: every word that is stored or compared stays canonical.  DerivedRegs<false> keeps canonical words for the run-time form.
template <bool CENTRED>
struct DerivedRegs {
    using word = std::conditional_t<CENTRED, i32, uint32_t>;
    BX_HD static word enter(uint32_t v) {
        if constexpr (CENTRED) return fp_centre(v);
        else return v;
    }
    word ring[8], u[3], k[4];
    // the pool of the column the walk stands at
    BX_HD void fill(word (&pool)[Circuit::POOL], word slot1) const {
        pool[0] = u[0]; pool[1] = slot1; pool[2] = u[1]; pool[3] = u[2];
#pragma unroll
        for (int q = 0; q < 8; ++q) pool[4 + q] = ring[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) pool[12 + q] = k[q];
    }
    // on to column j+1: d = the value of column F+j, next_u = free column (j+3) mod F, next_k = code csel(j+4)
    BX_HD void shift(word d, word next_u, word next_k) {
#pragma unroll
        for (int q = 7; q > 0; --q) ring[q] = ring[q - 1];
        ring[0] = d;
        u[0] = u[1]; u[1] = u[2]; u[2] = next_u;
        k[0] = k[1]; k[1] = k[2]; k[2] = k[3]; k[3] = next_k;
    }
};

}  // inline namespace BX_MAD_FLAVOUR
}  // namespace bx
