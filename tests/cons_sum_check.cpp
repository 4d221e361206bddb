// cons_sum_check.cpp — CPU check of the constraint sums of boundless_amd/csrc/circuit_dev.hpp, the core of witness_derive_kernel and
// eval_check_kernel: cons_sum<TT, GG> carries a cell's sum in one 64-bit chain that is never reduced on the way, only folded
// (a -> hi(a) * R + lo(a), fold_r), and reduced once at the end.  Checked here:
//   (a) fold_r: congruent to its operand mod P and inside |a|/16 + 2^32 + R, at +-(2^63 - 1), +-(the steady-state maximum of a chain),
//       0, -1, a low word of 0xFFFFFFFF under either sign of the high word, and random operands;
//   (b) the plans that run: FoldPlan<TT> (G = 4: every term once, under the two pairs PairPlan chose for it, which multiply to exactly
//       its four pool entries; the pairs distinct, each computed at its first use; no segment beyond SEG terms or with a pair in common;
//       the chain and total bounds recomputed here from the segment sizes) and ConsPlan<TT, GG> (G = 3, G >= 5: every term once, under
//       its own first factor; no pool entry twice in a segment; the chain bound recomputed);
//   (c) cons_sum<TT, GG> for every shape circuit.hip dispatches — (64,4), (48,3), (16,3), (8,2) — and for term counts that leave the
//       groups and segments uneven, longer products (G = 5) and G = 1, through the centred entry and through the canonical-pool
//       signature, against the run-time term-by-term loop cons_sum<0, 0>: all 2^16 pools whose entries are +-P/2 (the all-positive
//       pool among them, where a chain is largest), pools of 0, P - 1, P/2, P/2 + 1, edge words mixed with random ones, random pools;
//   (d) a walk of 19 derived cells (two runs of eight and three more: slot 1 is a back-tap at j = 0, 4, 8, 12, 16) through
//       DerivedRegs<true>, entries centred where they are loaded or produced, against the same walk through DerivedRegs<false> with
//       canonical entries and the term-by-term loop: the pool and the value of every cell.
// Built by tests/test_cons_sum_cpu.py plainly, with -DBX_CHECK_BOUNDS (every pool entry, pair, sredc operand, fold_r operand and
// result, chain and total is asserted against its bound; run with the argument `uncentred` the program hands over one entry of
// P/2 + 1, which that build must refuse) and with the bounds under -fsanitize=address,undefined, where a chain that left 64 bits
// would be a signed overflow; a stand-alone program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "fp.hpp"
#include "poseidon2_arith.hpp"
#include "circuit_dev.hpp"

using namespace bx;

static uint64_t rng_state = 0xA4093822299F31D0ull;
static uint64_t rnd64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static const uint32_t HALF = P / 2, NHALF = P / 2 + 1;  // centred: +P/2 and -P/2
static const int EDGE_POOLS = 40000, RANDOM_POOLS = 120000, RANDOM_FOLDS = 1000000, RANDOM_WALKS = 400, WALK = 19;

// ---- (a) the fold ------------------------------------------------------------------------------------------------------------
static uint32_t mod_p(i64 v) {
    const i64 r = v % (i64)P;
    return (uint32_t)(r < 0 ? r + (i64)P : r);
}
static int check_fold(i64 a) {
    const i64 r = fold_r(a);
    const i64 mag = a < 0 ? -a : a, rmag = r < 0 ? -r : r;
    if (mod_p(r) != mod_p(a)) {
        fprintf(stderr, "fold_r(%lld) = %lld is not congruent mod P\n", (long long)a, (long long)r);
        return 1;
    }
    if (rmag > mag / 16 + ((i64)1 << 32) + (i64)MONT_ONE || rmag > fold_ub(mag)) {
        fprintf(stderr, "fold_r(%lld) = %lld is beyond |a|/16 + 2^32 + R\n", (long long)a, (long long)r);
        return 1;
    }
    return 0;
}
static int check_folds() {
    const i64 steady = FoldPlan<64>::STEADY;
    const i64 fixed[] = {INT64_MAX, -INT64_MAX, steady, -steady, 0, -1, 1, (i64)0xFFFFFFFFll, ((i64)0x7FFFFFFF << 32) | (i64)0xFFFFFFFFll,
                         -((i64)1 << 32) + (i64)0xFFFFFFFFll /* hi = -1 */, (i64)((uint64_t)0x80000001u << 32 | 0xFFFFFFFFu) /* hi = -(2^31 - 1) */,
                         INT64_MIN + (i64)0xFFFFFFFFll /* hi = -2^31 */, (i64)1 << 32, -((i64)1 << 32), SREDC_MAX, -SREDC_MAX, FINAL_MAX, -FINAL_MAX};
    for (i64 a : fixed)
        if (check_fold(a)) return 1;
    for (int i = 0; i < RANDOM_FOLDS; ++i) {
        i64 a = (i64)rnd64();
        if (i & 1) a >>= (rnd64() % 40);  // small magnitudes too
        if (a == INT64_MIN) a = -INT64_MAX;
        if (check_fold(a)) return 1;
    }
    // a steady-state chain folds to well inside the last reduction's range: the end of every cons_sum
    if (fold_ub(steady) > FINAL_MAX || steady >= INT64_MAX) {
        fprintf(stderr, "steady-state chain %lld folds to %lld, FINAL_MAX %lld\n", (long long)steady, (long long)fold_ub(steady), (long long)FINAL_MAX);
        return 1;
    }
    return 0;
}

// ---- (b) the plans -----------------------------------------------------------------------------------------------------------
#define FAIL(...)                                            \
    do {                                                     \
        fprintf(stderr, "%s: ", what);                       \
        fprintf(stderr, __VA_ARGS__);                        \
        fprintf(stderr, "\n");                               \
        return 1;                                            \
    } while (0)

template <int TT>
static int check_fold_plan() {
    char what[64];
    snprintf(what, sizeof what, "FoldPlan<%d>", TT);
    using Plan = FoldPlan<TT>;
    using Pairs = PairPlan<TT>;
    const Plan& plan = fold_plan<TT>;
    const Pairs& pairs = pair_plan<TT>;
    constexpr int SEG = Plan::SEG;
    // as many pairs as PairPlan's choice of splits holds distinct ones
    bool chosen[Pairs::NID] = {false};
    int distinct = 0;
    for (int t = 0; t < TT; ++t)
        for (int k = 0; k < 2; ++k) {
            const int id = pairs.pair[t][k];
            if (id < 0 || id >= Pairs::NID) FAIL("PairPlan gives term %d the pair id %d", t, id);
            if (!chosen[id]) chosen[id] = true, ++distinct;
        }
    if (plan.np != distinct) FAIL("%d pairs, PairPlan's splits hold %d distinct ones", plan.np, distinct);
    if (plan.pbeg[0] != 0 || plan.pbeg[TT] != plan.np) FAIL("first uses end at %d of %d", plan.pbeg[TT], plan.np);
    for (int p = 0; p < plan.np; ++p) {
        if (plan.pa[p] < 0 || plan.pa[p] > plan.pb[p] || plan.pb[p] >= (int)Circuit::POOL) FAIL("pair %d = (%d, %d)", p, plan.pa[p], plan.pb[p]);
        for (int q = 0; q < p; ++q)
            if (plan.pa[q] == plan.pa[p] && plan.pb[q] == plan.pb[p]) FAIL("pairs %d and %d are the same product", q, p);
    }
    int seen[TT] = {0}, used[2 * TT] = {0};
    for (int s = 0; s < TT; ++s) {
        const int t = plan.seq[s];
        if (t < 0 || t >= TT || seen[t]++) FAIL("slot %d holds term %d wrongly", s, t);
        if (plan.pbeg[s + 1] < plan.pbeg[s]) FAIL("first uses run backwards at slot %d", s);
        int want[4], got[4];
        for (unsigned f = 0; f < 4; ++f) want[f] = (int)Circuit::pool_idx((unsigned)t, f);
        for (int k = 0; k < 2; ++k) {
            const int p = k ? plan.s2[s] : plan.s1[s];
            if (p < 0 || p >= plan.pbeg[s + 1]) FAIL("slot %d uses pair %d before it is computed (%d so far)", s, p, plan.pbeg[s + 1]);
            if (Pairs::pair_id((unsigned)plan.pa[p], (unsigned)plan.pb[p]) != pairs.pair[t][k]) FAIL("slot %d: pair %d = (%d, %d) is not the one PairPlan chose for term %d", s, p, plan.pa[p], plan.pb[p], t);
            ++used[p];
            got[2 * k] = plan.pa[p];
            got[2 * k + 1] = plan.pb[p];
        }
        std::sort(want, want + 4);
        std::sort(got, got + 4);
        if (!std::equal(want, want + 4, got)) FAIL("term %d = {%d,%d,%d,%d}, its pairs give {%d,%d,%d,%d}", t, want[0], want[1], want[2], want[3], got[0], got[1], got[2], got[3]);
    }
    for (int p = 0; p < plan.np; ++p) {
        if (!used[p]) FAIL("pair %d is never used", p);
        int s = 0;
        while (plan.pbeg[s + 1] <= p) ++s;
        if (plan.s1[s] != p && plan.s2[s] != p) FAIL("pair %d is computed at slot %d, which does not use it", p, s);
    }
    if (plan.ns < 1 || plan.sbeg[0] != 0 || plan.sbeg[plan.ns] != TT) FAIL("%d segments end at slot %d", plan.ns, plan.sbeg[plan.ns]);
    // the bounds, from the segment sizes alone: the first segment starts from nothing, every later one from the folded chain
    i64 chain = 0, max_chain = 0;
    for (int g = 0; g < plan.ns; ++g) {
        const int b = plan.sbeg[g], e = plan.sbeg[g + 1];
        if (e <= b || e - b > SEG) FAIL("segment %d holds %d terms", g, e - b);
        for (int s = b; s < e; ++s)
            for (int r = b; r < s; ++r)
                if (plan.s1[s] == plan.s1[r] || plan.s1[s] == plan.s2[r] || plan.s2[s] == plan.s1[r] || plan.s2[s] == plan.s2[r]) FAIL("segment %d: slots %d and %d share a pair", g, r, s);
        const i64 start = g == 0 ? 0 : fold_ub(chain), add = (i64)(e - b) * Plan::TERM;
        if (start > INT64_MAX - add) FAIL("segment %d takes the chain beyond 2^63", g);
        chain = start + add;
        max_chain = std::max(max_chain, chain);
    }
    const i64 total = fold_ub(chain);
    if (max_chain != plan.max_chain || total != plan.max_total) FAIL("bounds: chain %lld (plan %lld), total %lld (plan %lld)", (long long)max_chain, (long long)plan.max_chain, (long long)total, (long long)plan.max_total);
    if (max_chain > Plan::STEADY || Plan::STEADY >= INT64_MAX || total > FINAL_MAX || FINAL_MAX > SREDC_MAX) FAIL("bounds: chain %lld, steady %lld, total %lld", (long long)max_chain, (long long)Plan::STEADY, (long long)total);
    if (ub(total) >= (i64)P) FAIL("the last reduction can reach P in magnitude");
    // the steady-state bound is one: a chain at it, folded, plus a full segment stays at or below it
    if (fold_ub(Plan::STEADY) + SEG * Plan::TERM > Plan::STEADY) FAIL("STEADY is not invariant");
    const double p2 = (double)P * (double)P;
    printf("%s: %d pairs, %d segments, at most %d pairs alive, chain <= %.4f P^2, total <= %.4f P^2\n", what, plan.np, plan.ns, plan.max_live, (double)max_chain / p2, (double)total / p2);
    if (TT == 64 && plan.np > 51) FAIL("%d distinct pairs, more than 51", plan.np);
    if (TT == 64 && plan.ns != (TT + SEG - 1) / SEG) FAIL("%d segments where %d would do", plan.ns, (TT + SEG - 1) / SEG);
    return 0;
}

template <int TT, int GG>
static int check_cons_plan() {
    char what[64];
    snprintf(what, sizeof what, "ConsPlan<%d, %d>", TT, GG);
    using Plan = ConsPlan<TT, GG>;
    const Plan& plan = cons_plan<TT, GG>;
    if (plan.nf < 1 || plan.fbeg[0] != 0 || plan.fbeg[plan.nf] != plan.nq) FAIL("%d fold segments end at inner group %d of %d", plan.nf, plan.fbeg[plan.nf], plan.nq);
    i64 cur = 0, max_chain = 0;
    int seen[TT] = {0}, terms = 0;
    for (int f = 0; f < plan.nf; ++f) {
        if (plan.fbeg[f + 1] <= plan.fbeg[f]) FAIL("fold segment %d is empty", f);
        if (f > 0) cur = fold_ub(cur);
        for (int q = plan.fbeg[f]; q < plan.fbeg[f + 1]; ++q) {
            for (int r = plan.fbeg[f]; r < q; ++r)
                if (plan.first[r] == plan.first[q]) FAIL("fold segment %d holds pool entry %d twice", f, plan.first[q]);
            // the grouping itself: every term exactly once, under its own first factor
            for (int k = 0; k < plan.len[q]; ++k) {
                const int t = plan.term[q][k];
                if (t < 0 || t >= TT || (int)Circuit::pool_idx((unsigned)t, 0u) != plan.first[q] || seen[t]++) FAIL("inner group %d holds term %d wrongly", q, t);
            }
            const i64 add = ub(plan.len[q] * Plan::TERM) * Plan::BC;
            if (plan.len[q] * Plan::TERM > SREDC_MAX || cur > INT64_MAX - add) FAIL("inner group %d takes the chain beyond 2^63", q);
            cur += add;
            max_chain = std::max(max_chain, cur);
            terms += plan.len[q];
        }
    }
    if (terms != TT || max_chain != plan.max_fchain || fold_ub(cur) != plan.max_ftotal || plan.max_ftotal > FINAL_MAX) FAIL("%d terms, chain %lld (plan %lld), folded %lld (plan %lld)", terms, (long long)max_chain, (long long)plan.max_fchain, (long long)fold_ub(cur), (long long)plan.max_ftotal);
    const double p2 = (double)P * (double)P;
    printf("%s: %d inner groups, %d fold segments, chain <= %.4f P^2, folded <= %.4f P^2\n", what, plan.nq, plan.nf, (double)max_chain / p2, (double)plan.max_ftotal / p2);
    return 0;
}

// ---- (c) the values ----------------------------------------------------------------------------------------------------------
template <int TT, int GG>
static int check_one(const uint32_t (&pool_u)[Circuit::POOL], const char* what, long iter) {
    i32 pool_c[Circuit::POOL];
    for (unsigned i = 0; i < Circuit::POOL; ++i) {
        pool_c[i] = fp_centre(pool_u[i]);
        if (pool_c[i] > (i32)(P / 2) || pool_c[i] < -(i32)(P / 2) || (uint32_t)(pool_c[i] + (pool_c[i] < 0 ? (i32)P : 0)) != pool_u[i]) {
            fprintf(stderr, "fp_centre(%u) = %d\n", pool_u[i], pool_c[i]);
            return 1;
        }
    }
    const uint32_t want = cons_sum<0, 0>(pool_u, TT, GG), got = cons_sum<TT, GG>(pool_c, TT, GG), canon = cons_sum<TT, GG>(pool_u, TT, GG);
    if (got != want || canon != want || got >= P) {
        fprintf(stderr, "cons_sum<%d,%d> mismatch on %s pool %ld: centred entry %u, canonical entry %u, term by term %u\n", TT, GG, what, iter, got, canon, want);
        return 1;
    }
    return 0;
}

template <int TT, int GG>
static int check_shape() {
    uint32_t pool[Circuit::POOL];
    for (long signs = 0; signs < (1l << Circuit::POOL); ++signs) {   // every entry +-P/2; signs = 0 is the all-positive pool
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = ((signs >> i) & 1) ? NHALF : HALF;
        if (check_one<TT, GG>(pool, "sign-pattern", signs)) return 1;
    }
    const uint32_t fills[] = {0u, P - 1, HALF, NHALF};
    for (int m = 0; m < 4; ++m) {
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = fills[m];
        if (check_one<TT, GG>(pool, "constant", m)) return 1;
    }
    // edge words mixed with random ones
    const uint32_t edge[] = {0, 1, P - 1, HALF, NHALF, HALF - 1, MONT_ONE, P - MONT_ONE};
    for (long iter = 0; iter < EDGE_POOLS; ++iter) {
        for (unsigned i = 0; i < Circuit::POOL; ++i) {
            const uint64_t r = rnd64();
            pool[i] = (r & 1) ? edge[(r >> 8) % 8] : (uint32_t)((r >> 8) % P);
        }
        if (check_one<TT, GG>(pool, "edge-mix", iter)) return 1;
    }
    for (long iter = 0; iter < RANDOM_POOLS; ++iter) {
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = (uint32_t)(rnd64() % P);
        if (check_one<TT, GG>(pool, "random", iter)) return 1;
    }
    return 0;
}

// ---- (d) the walk ------------------------------------------------------------------------------------------------------------
// modes 0..4 are the fixed words (all P/2, all P/2 + 1, alternating, 0, P - 1), anything else is random
static void make_words(uint32_t* w, int n, int mode) {
    for (int i = 0; i < n; ++i)
        w[i] = mode == 0 ? HALF : mode == 1 ? NHALF : mode == 2 ? ((i & 1) ? NHALF : HALF) : mode == 3 ? 0u : mode == 4 ? P - 1 : (uint32_t)(rnd64() % P);
}

// One row of a trace as the walk sees it: F free columns, a back-tap per derived column, code selectors (or the constant one).
struct Row {
    static const int F = 5, NCODE = 3;  // five free columns: j+1, j+2 and (j+3) % F wrap inside the walk
    uint32_t free_col[F], back[WALK], code[NCODE];
    bool const_one;                     // fewer than three code columns: every csel is the constant one
    uint32_t code_at(unsigned i) const { return const_one ? MONT_ONE : code[i % NCODE]; }
};

// the walk of circuit.hip's two kernels on one row, the derived values of its WALK cells into out[]; on the way the pool of every
// cell is handed to `seen` as canonical words
template <bool CENTRED, int TT, int GG>
static void walk(const Row& row, uint32_t (&out)[WALK], uint32_t (&seen)[WALK][Circuit::POOL]) {
    using Regs = DerivedRegs<CENTRED>;
    using word = typename Regs::word;
    Regs w;
    for (int q = 0; q < 8; ++q) w.ring[q] = Regs::enter(row.code_at((unsigned)q));
    for (int q = 0; q < 3; ++q) w.u[q] = Regs::enter(row.free_col[q % Row::F]);
    for (int q = 0; q < 4; ++q) w.k[q] = Regs::enter(row.code_at((unsigned)q));
    for (uint32_t j = 0; j < (uint32_t)WALK; ++j) {
        word pool[Circuit::POOL];
        w.fill(pool, Circuit::slot1_back(j) == 0 ? w.u[0] : Regs::enter(row.back[j]));
        for (unsigned i = 0; i < Circuit::POOL; ++i) seen[j][i] = (uint32_t)pool[i] + ((int64_t)pool[i] < 0 ? P : 0u);
        const uint32_t d = cons_sum<TT, GG>(pool, (uint32_t)(TT ? TT : 64), (uint32_t)(GG ? GG : 4));
        out[j] = d;
        w.shift(Regs::enter(d), Regs::enter(row.free_col[(j + 3) % Row::F]), Regs::enter(row.code_at(j + 4)));
    }
}

static int check_walk(int mode, int iter, bool const_one) {
    Row row;
    make_words(row.free_col, Row::F, mode);
    make_words(row.back, WALK, mode);
    make_words(row.code, Row::NCODE, mode);
    row.const_one = const_one;
    uint32_t want[WALK], got[WALK], pools_want[WALK][Circuit::POOL], pools_got[WALK][Circuit::POOL];
    walk<false, 0, 0>(row, want, pools_want);
    walk<true, 64, 4>(row, got, pools_got);
    for (int j = 0; j < WALK; ++j) {
        for (unsigned i = 0; i < Circuit::POOL; ++i)
            if (pools_got[j][i] != pools_want[j][i]) {
                fprintf(stderr, "walk mode %d iteration %d: pool entry %u of cell %d is %u through the centred registers, %u through the canonical ones\n", mode,
                        iter, i, j, pools_got[j][i], pools_want[j][i]);
                return 1;
            }
        if (got[j] != want[j] || got[j] >= P) {
            fprintf(stderr, "walk mode %d iteration %d: cell %d is %u through the centred registers, %u through the canonical ones\n", mode, iter, j, got[j],
                    want[j]);
            return 1;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "uncentred")) {
        // one entry a single step outside [-P/2, P/2]: a build with BX_CHECK_BOUNDS must refuse it (the test expects the abort)
        i32 pool[Circuit::POOL];
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = (i32)HALF;
        pool[5] = (i32)NHALF;
        printf("cons_sum<64,4> took an entry of P/2 + 1: %u\n", cons_sum<64, 4>(pool, 64, 4));
        return 0;
    }
    if (check_folds()) return 1;
    if (check_fold_plan<64>() || check_fold_plan<33>() || check_fold_plan<17>() || check_fold_plan<7>() || check_fold_plan<1>()) return 1;
    if (check_cons_plan<48, 3>() || check_cons_plan<16, 3>() || check_cons_plan<32, 3>() || check_cons_plan<33, 3>() || check_cons_plan<64, 5>() ||
        check_cons_plan<7, 3>())
        return 1;
    // the dispatched shapes (circuit.hip: BX_CIRCUIT_DISPATCH), then term counts that leave the last group or segment short, G = 5, G = 1
    if (check_shape<64, 4>() || check_shape<48, 3>() || check_shape<16, 3>() || check_shape<8, 2>()) return 1;
    if (check_shape<33, 4>() || check_shape<17, 4>() || check_shape<7, 4>() || check_shape<1, 4>() || check_shape<33, 3>() || check_shape<64, 5>() ||
        check_shape<25, 2>() || check_shape<9, 2>() || check_shape<17, 1>() || check_shape<1, 1>())
        return 1;
    for (int c = 0; c < 2; ++c) {
        for (int mode = 0; mode < 5; ++mode)
            if (check_walk(mode, 0, c != 0)) return 1;
        for (int iter = 0; iter < RANDOM_WALKS; ++iter)
            if (check_walk(5, iter, c != 0)) return 1;
    }
    printf("cons_sum_check ok\n");
    return 0;
}
