// circuit_dev.hpp — the arithmetic core shared by witness generation and eval_check: the value of one derived cell,
//     sum_{t<T} prod_{f<G} pool[idx(t,f)]            (include/bx_prover.h, "The synthetic circuit")
// Both knobs are compile-time for the shapes the prover is tuned for (every pool reference is then a fixed register);
// <0, 0> is the run-time fallback for any other (T, G) and uses plain canonical arithmetic.
//
// The arithmetic.  The compile-time paths run on the signed, bounded Montgomery arithmetic of poseidon2_arith.hpp (sredc(t) =
// (t + mP)/2^32, |result| <= ub(|t|) = |t|/2^32 + P/2 + 1, valid for |t| <= SREDC_MAX = 1.209 P^2; P^2/2^32 = 0.469 P), so that no
// product is followed by a conditional subtraction and the sums stay unreduced in 64 bits.  Pool entries are centred, |c| <= P/2: by
// the walk of circuit.hip once per word, where it enters the registers (DerivedRegs<true> and the centred entry of cons_sum; 4 of the
// 16 entries are new per cell), by the canonical-pool signature once per call.
//
// The chain.  The sum of a cell's terms is one signed 64-bit accumulator that is never reduced on the way.  Where it would leave 64
// bits it is FOLDED, a = hi * 2^32 + lo  ->  hi * R + lo (fold_r; R = 2^32 mod P = 2^28 - 2, so the value is congruent mod P and
// |result| <= |a|/16 + 2^32 + R): one v_mad_i64_i32 and the copy that puts lo beside a zero register.  The terms carry one factor R
// more than the result; the one sredc at the end, of the folded chain, takes it away.
//   a chain               A <= fold_ub(A) + (the terms of a segment), with the segments cut so that A < 2^63 = 2.2755 P^2
//   the end               result = sredc(fold_r(A)):  fold_ub(A) <= 0.14 P^2 + 2^32 <= FINAL_MAX, so |result| < P, one conditional
//                         add of P makes it canonical, and the word is the one the run-time loop gives
// Two fences keep hipcc from undoing this where the multiply-adds are the compiler's (BX_PLAIN_MAD, as in circuit.hip).  smad_chain
// hides each step's result behind an empty asm (no instruction): in sight, hipcc reassociates fold + t1 + ... + tn into
// fold + (t1 + ... + tn) and pays a 64-bit add per segment, and it rewrites two terms with a common factor, p*q1 + p*q2, as
// p*(q1 + q2) with a 64-bit sum and an emulated 64 x 32-bit product.  smad_r multiplies by an opaque signed copy of R, one per use:
// with the constant in sight hipcc rewrites a sum of r_i * R as (sum of r_i) * R, again with an emulated product, and takes a single
// r * R apart into shifts.  Compiled, the walk's loop body per cell, VALU instructions / multiplies (v_mad_i64_i32 + v_mul_lo_u32 +
// v_mad_u64_u32): witness_derive_kernel<64,4> 262 / 211 (46 VGPRs), eval_check_kernel<64,4> 317 / 235 (70 VGPRs: seven waves per
// SIMD); (48, 3) 144 / 102, (16, 3) 110 / 69, (8, 2) 49 / 11; no scratch, no v_mad_u64_u32 in any of them.
//
// G = 4, the pair form.  A term is a product of four pool entries and can be written as (pair) * (pair) in three ways.  PairPlan
// picks one split per term so that pairs recur (44 distinct pairs serve the 128 pair slots of T = 64), and a term is ONE multiply-add
// of two shared, reduced pair products.  PairPlan carries that choice and nothing else: per term, the ids of its two pairs.
// FoldPlan is what cons_sum executes: it numbers the pairs by first use, orders the terms into segments (13 at T = 64) so that a
// pair's uses lie close together (at most 11 pairs are computed and still awaited at any point of T = 64), and carries the bounds.
//   a pair                p = sredc(c_a * c_b), computed at its first use:   |p| <= ub(P^2/4) = 0.617 P
//   a term                p1 * p2:                                           |t| <= 0.381 P^2
//   a segment             <= SEG = 5 terms added to the chain after its fold: A <= A/16 + 5 * 0.381 P^2, A <= 2.033 P^2 (six: 2.44 P^2)
//                         no two terms of a segment share a pair (the rewrite above, should a step ever be left in sight)
//
// G = 3 and G >= 5, the factored form.  pool_idx(t, 0) runs through all 16 pool entries on every block of 16 terms, so entry a is the
// first factor of T/16 terms and   sum_{t: idx(t,0)=a} pool[a] * (rest of t)  =  pool[a] * sum_t (rest of t):  the product with
// pool[a] is taken once per group of terms instead of once per term.  ConsPlan carries the inner groups (their shared first factor,
// their terms), the fold segments they are dealt into, and the bound of every accumulator.
//   the rest of a term    y = pool[idx(t,1)],  y <- sredc(y * pool[idx(t,f)]) for f = 2 .. G-2,  then  y * pool[idx(t,G-1)]:
//                         G = 3: |y| <= 0.5 P, term <= 0.25 P^2;   G >= 5: |y| <= 0.65 P for any chain length, term <= 0.325 P^2
//   inner group           inner = sum of <= ISZ terms with the same first factor:  G = 3: ISZ = 4, |inner| <= 1.0 P^2;
//                         G >= 5: ISZ = 3 (four terms would leave SREDC_MAX).  An entry with more terms than ISZ gets several inner
//                         groups of balanced size
//   its reduction         s = sredc(inner):   G = 3: |s| <= 0.97 P (4 terms), 0.85 P (3)
//   the chain             A = sum of s * pool[a] over the inner groups, folded in front of each fold segment: as few segments as
//                         keep A < 2^63, the groups spread evenly over them, no pool entry twice in a segment
//                         ((48, 3): 16 groups in 4 segments of 4, A <= 1.82 P^2)
//
// G <= 2 has no shared product to factor out: one chain of the terms x * c_last (<= 0.25 P^2 each) in their order, folded in front of
// every eighth: A <= A/16 + 8 * 0.25 P^2, A <= 2.134 P^2.
//
// cons_sum's static_asserts hold every plan to SREDC_MAX / FINAL_MAX and the chains to their steady-state bound; the host build
// (BX_CHECK_BOUNDS) asserts every pool entry, pair, sredc operand, fold operand and result, and every chain after every segment
// (tests/cons_sum_check.cpp).  Tests compare every form with the run-time loop and with the oracle.
#pragma once
#include <type_traits>

#include "circuit.hpp"
#include "fp.hpp"
#include "lazy_ext.hpp"  // smad_r, fold_r, smad_chain, FINAL_MAX: the chain steps and the fold
#include "poseidon2_arith.hpp"

namespace bx {
inline namespace BX_MAD_FLAVOUR {

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

    int nq = 0;                            // inner groups
    int first[TT]{}, len[TT]{}, term[TT][ISZ]{};  // inner group q: its shared first factor, its terms
    i64 max_inner = 0;                     // the largest inner sum
    // ONE chain over all inner groups' s * pool[a], folded (fold_r) at the head of every segment but the first
    int nf = 0, fbeg[TT + 1]{};            // segment f = inner groups [fbeg[f], fbeg[f+1])
    i64 max_fchain = 0, max_ftotal = 0;    // the largest chain value, the folded chain that is reduced at the end

    constexpr ConsPlan() {
        // inner groups in the order (g, a): the g-th group of every pool entry before any (g+1)-th, so that neighbours in the chain
        // are groups of different entries (cut_segments)
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
        // the fold segments: as few as the bound allows (a cut wherever the next group would take the chain beyond 64 bits),
        // then the same number of segments with the groups spread evenly, which leaves the chain the most room
        const int fewest = cut_segments(nq);
        if (cut_segments((nq + fewest - 1) / fewest) > fewest) cut_segments(nq);
    }
    // fills nf, fbeg and the chain's bounds: at most `cap` consecutive inner groups to a segment, fewer where the chain would leave
    // 64 bits or a pool entry would come twice (hipcc would add the two reductions first and emulate a 64 x 32-bit product for the sum)
    constexpr int cut_segments(int cap) {
        i64 cur = 0;
        nf = 0;
        max_fchain = 0;
        for (int q = 0; q < nq; ++q) {
            const i64 add = ub(len[q] * TERM) * BC;
            bool again = false;
            for (int r = fbeg[nf]; r < q; ++r) again = again || first[r] == first[q];
            if (q > 0 && (again || q - fbeg[nf] >= cap || cur > INT64_MAX - add)) {
                fbeg[++nf] = q;
                cur = fold_ub(cur);
            }
            cur += add;
            if (cur > max_fchain) max_fchain = cur;
        }
        fbeg[++nf] = nq;
        max_ftotal = fold_ub(cur);
        return nf;
    }
};
template <int TT, int GG>
inline constexpr ConsPlan<TT, GG> cons_plan{};

// The choice of the pair form (G = 4) for one T: which of its three splits into two pairs each term takes.
template <int TT>
struct PairPlan {
    static constexpr int NPOOL = (int)Circuit::POOL, NID = NPOOL * NPOOL;
    static constexpr i64 BC = (i64)(P / 2);                   // a centred pool entry
    static constexpr i64 PAIR = ub(BC * BC);                  // a reduced pair product
    static constexpr i64 TERM = PAIR * PAIR;                  // one term: a product of two pairs
    static constexpr int pair_id(unsigned a, unsigned b) { return a < b ? (int)(a * NPOOL + b) : (int)(b * NPOOL + a); }

    int pair[TT][2]{};                     // term t = pair pair[t][0] * pair pair[t][1], as pair_id; [0] holds the term's factor 0

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
        for (int t = 0; t < TT; ++t)
            for (int k = 0; k < 2; ++k) pair[t][k] = sp[t][ch[t]][k];
    }
};
template <int TT>
inline constexpr PairPlan<TT> pair_plan{};

// What cons_sum<TT, 4> executes: PairPlan's splits, the terms put into SEGMENTS of at most SEG on one chain, the pairs numbered by
// first use.  The chain is a 64-bit accumulator that is never reduced on the way: before a segment adds its terms the chain is
// folded, a -> hi(a) * R + lo(a) (fold_r), which is congruent mod P and sixteen times smaller.
//   a term                |p1 * p2| <= TERM = 0.381 P^2                                    (2^63 = 2.2755 P^2)
//   the chain             A <= fold_ub(A) + SEG * TERM = A/16 + 5 * 0.381 P^2:  A <= 2.033 P^2 < 2^63  (six terms: 2.44 P^2)
//   the total             the folded chain <= 0.127 P^2 + 2^32 + R <= FINAL_MAX, so its reduction is < P
// The order is greedy: the next term is the one that needs the fewest pairs not yet computed, then the one that uses the most pairs
// for the last time, so that a pair's uses lie close together; candidates are taken by rising term index and only a strictly better
// one replaces the choice.  No two terms of a segment share a pair (hipcc would rewrite p*q1 + p*q2 as p*(q1 + q2) with a 64-bit sum
// and an emulated product).  One rule comes first: a pair with as many uses left as segments left goes into the current segment, or
// its last users end up in short segments of their own (T = 64: 17 segments without the rule, the last four of one term; 13 with it).
// One chain: segments dealt over two or three were tried and cost instructions, time or a wave (tools/experiments/README.md).
template <int TT>
struct FoldPlan {
    static constexpr int SEG = 5, NPOOL = PairPlan<TT>::NPOOL, NID = PairPlan<TT>::NID;
    static constexpr i64 TERM = PairPlan<TT>::TERM;
    // the chain bound with every segment full, however many segments: fold_ub(A) <= A/16 + R + 2^32, so 16/15 of the rest holds
    static constexpr i64 STEADY = (SEG * TERM + (i64)MONT_ONE + ((i64)1 << 32)) / 15 * 16 + 16;
    static_assert(STEADY < INT64_MAX && fold_ub(STEADY) + SEG * TERM <= STEADY, "cons_sum: the chain bound is not invariant below 2^63");

    int np = 0, ns = 0;                    // distinct pairs, segments
    int pa[2 * TT]{}, pb[2 * TT]{};        // pair p = pool[pa[p]] * pool[pb[p]], numbered by first use
    int seq[TT]{}, s1[TT]{}, s2[TT]{};     // slot s sums term seq[s] = pair s1[s] * pair s2[s]
    int pbeg[TT + 1]{};                    // pairs [pbeg[s], pbeg[s+1]) are computed at slot s, their first use
    int sbeg[TT + 1]{};                    // segment g = slots [sbeg[g], sbeg[g+1])
    int max_live = 0;                      // most pairs computed and still to be used at any slot
    i64 max_chain = 0, max_total = 0;      // the largest chain value, the folded chain that is reduced at the end

    constexpr FoldPlan() {
        const PairPlan<TT>& pp = pair_plan<TT>;
        int ref[NID]{}, num[NID]{};        // by pair id: uses left, number (-1 until its first use)
        for (int t = 0; t < TT; ++t) {
            ++ref[pp.pair[t][0]];
            ++ref[pp.pair[t][1]];
        }
        for (int i = 0; i < NID; ++i) num[i] = -1;
        int live = 0, glen = 0, gp[2 * SEG]{};
        bool placed[TT]{};
        for (int slot = 0; slot < TT;) {
            int best = -1, best_new = 3, best_last = -1, best_due = 0;
            const int segs_left = (TT - slot + glen + SEG - 1) / SEG;   // this segment and the full ones the other terms would fill
            if (glen < SEG)
                for (int t = 0; t < TT; ++t) {
                    if (placed[t]) continue;
                    const int a = pp.pair[t][0], b = pp.pair[t][1];
                    bool clash = false;
                    for (int k = 0; k < 2 * glen; ++k) clash = clash || gp[k] == a || gp[k] == b;
                    if (clash) continue;
                    // a pair with as many uses left as segments left must be used in every one of them, or segments get added at the end
                    const int most = ref[a] > ref[b] ? ref[a] : ref[b], due = most >= segs_left ? most : 0;
                    const int fresh = (num[a] < 0) + (num[b] < 0 && b != a);
                    const int last = a == b ? (ref[a] == 2) : (ref[a] == 1) + (ref[b] == 1);
                    if (due > best_due || (due == best_due && (fresh < best_new || (fresh == best_new && last > best_last))))
                        best = t, best_new = fresh, best_last = last, best_due = due;
                }
            if (best < 0) {                // the segment is full, or every term left shares a pair with it
                sbeg[++ns] = slot;
                glen = 0;
                continue;
            }
            const int a = pp.pair[best][0], b = pp.pair[best][1];
            for (int k = 0; k < 2; ++k) {  // both new: the pair that holds the term's factor 0 gets the lower number
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
        sbeg[++ns] = TT;
        i64 a = 0;
        for (int g = 0; g < ns; ++g) {     // the chain: folded (but for the first segment), then this segment's terms on top
            a = (g == 0 ? 0 : fold_ub(a)) + (sbeg[g + 1] - sbeg[g]) * TERM;
            if (a > max_chain) max_chain = a;
        }
        max_total = fold_ub(a);
    }
};
template <int TT>
inline constexpr FoldPlan<TT> fold_plan{};

// The compile-time paths, on a pool that is already centred: |pool[i]| <= P/2 is what every bound of the plans rests on, and the
// host build (BX_CHECK_BOUNDS) asserts it for every entry.  The walk of circuit.hip calls this with the pool its DerivedRegs<true>
// keep centred from cell to cell; the canonical-pool signature below centres and forwards.
template <int TT, int GG>
BX_HD uint32_t cons_sum(const i32 (&pool)[Circuit::POOL], uint32_t /*T*/, uint32_t /*G*/) {
    static_assert(TT > 0 && GG > 0, "cons_sum: the run-time form takes a canonical pool");
#pragma unroll
    for (unsigned i = 0; i < Circuit::POOL; ++i) BX_ASSERT_BOUND(pool[i] <= (i32)(P / 2) && pool[i] >= -(i32)(P / 2), "cons_sum: a pool entry that is not centred");
    if constexpr (GG == 4) {
        static_assert(fold_plan<TT>.max_chain <= FoldPlan<TT>::STEADY, "cons_sum: the chain beyond its steady-state bound");
        static_assert(fold_plan<TT>.max_total <= FINAL_MAX, "cons_sum: the folded chain beyond the last reduction's range");
        // every index below is a constant expression, so each pool entry and each pair product is a fixed register
        i32 pr[fold_plan<TT>.np];
        i64 chain = 0;
        static_for<0, fold_plan<TT>.ns>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            static_for<fold_plan<TT>.sbeg[g], fold_plan<TT>.sbeg[g + 1]>([&](auto sc) {
                constexpr int s = decltype(sc)::value;
                static_for<fold_plan<TT>.pbeg[s], fold_plan<TT>.pbeg[s + 1]>([&](auto pc) {
                    constexpr int p = decltype(pc)::value;
                    pr[p] = sredc(smul(pool[fold_plan<TT>.pa[p]], pool[fold_plan<TT>.pb[p]], p), p);
                    BX_ASSERT_BOUND(pr[p] <= PairPlan<TT>::PAIR && pr[p] >= -PairPlan<TT>::PAIR, "cons_sum pair");
                });
                // a segment's first term goes on top of the folded chain (the first segment: on nothing), the others follow
                if constexpr (s > fold_plan<TT>.sbeg[g]) chain = smad_chain(pr[fold_plan<TT>.s1[s]], pr[fold_plan<TT>.s2[s]], chain, s);
                else if constexpr (g > 0) chain = smad_chain(pr[fold_plan<TT>.s1[s]], pr[fold_plan<TT>.s2[s]], fold_r(chain, g), s);
                else chain = smul(pr[fold_plan<TT>.s1[s]], pr[fold_plan<TT>.s2[s]], s);
            });
            BX_ASSERT_BOUND(chain <= fold_plan<TT>.max_chain && chain >= -fold_plan<TT>.max_chain, "cons_sum chain");
        });
        const i64 total = fold_r(chain, 0);
        BX_ASSERT_BOUND(total <= fold_plan<TT>.max_total && total >= -fold_plan<TT>.max_total, "cons_sum folded chain");
        const i32 result = sredc(total, 0);   // takes away the terms' surplus factor R
        return (uint32_t)(result + (result < 0 ? (i32)P : 0));
    } else if constexpr (GG >= 3) {
        static_assert(cons_plan<TT, GG>.max_inner <= SREDC_MAX, "cons_sum: a group sum beyond sredc's range");
        static_assert(cons_plan<TT, GG>.max_ftotal <= FINAL_MAX, "cons_sum: the folded chain beyond the last reduction's range");
        // every index below is a constant expression (static_for hands its counter over as a type), so each pool reference is a
        // fixed register; the chain is the one value that lives from group to group
        i64 chain = 0;
        static_for<0, cons_plan<TT, GG>.nf>([&](auto fc) {
            constexpr int f = decltype(fc)::value;
            static_for<cons_plan<TT, GG>.fbeg[f], cons_plan<TT, GG>.fbeg[f + 1]>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                i64 inner = 0;
                static_for<0, cons_plan<TT, GG>.len[q]>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    constexpr unsigned t = (unsigned)cons_plan<TT, GG>.term[q][k];
                    i32 y = pool[Circuit::pool_idx(t, 1u)];
#pragma unroll
                    for (int g = 2; g + 1 < GG; ++g) y = sredc(smul(y, pool[Circuit::pool_idx(t, (unsigned)g)], g), g);
                    inner = smad_chain(y, pool[Circuit::pool_idx(t, (unsigned)(GG - 1))], inner, k);
                });
                const i32 s = sredc(inner, 3);
                if constexpr (q > cons_plan<TT, GG>.fbeg[f]) chain = smad_chain(s, pool[cons_plan<TT, GG>.first[q]], chain, q);
                else if constexpr (f > 0) chain = smad_chain(s, pool[cons_plan<TT, GG>.first[q]], fold_r(chain, f), q);
                else chain = smul(s, pool[cons_plan<TT, GG>.first[q]], q);
            });
            BX_ASSERT_BOUND(iabs64(chain) <= (cons_plan<TT, GG>.max_fchain), "cons_sum chain");
        });
        const i32 result = sredc(fold_r(chain, 0), 0);
        return (uint32_t)(result + (result < 0 ? (i32)P : 0));
    } else {
        // one chain of the terms in their order, folded in front of every SEG2 of them: A <= A/16 + 8 * 0.25 P^2, A <= 2.134 P^2 < 2^63
        constexpr int SEG2 = 8;
        constexpr i64 TERM = (i64)(P / 2) * (GG == 1 ? (i64)MONT_ONE : (i64)(P / 2));
        constexpr i64 STEADY = (SEG2 * TERM + (i64)MONT_ONE + ((i64)1 << 32)) / 15 * 16 + 16;
        static_assert(GG >= 1 && STEADY < INT64_MAX && fold_ub(STEADY) + SEG2 * TERM <= STEADY && fold_ub(STEADY) <= FINAL_MAX, "cons_sum: the chain bound is not invariant below 2^63");
        i64 chain = 0;
        static_for<0, TT>([&](auto tc) {
            constexpr unsigned t = (unsigned)decltype(tc)::value;
            const i32 x = pool[Circuit::pool_idx(t, 0u)];
            if constexpr (t > 0 && t % SEG2 == 0) chain = fold_r(chain, (int)t);
            if constexpr (GG == 1) chain = smad_r(x, chain, (int)t);
            else if constexpr (t == 0) chain = smul(x, pool[Circuit::pool_idx(t, 1u)], 0);
            else chain = smad_chain(x, pool[Circuit::pool_idx(t, 1u)], chain, (int)t);
            BX_ASSERT_BOUND(chain <= STEADY && chain >= -STEADY, "cons_sum chain");
        });
        const i32 result = sredc(fold_r(chain, 0), 0);
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
