// cons_pairs_check.cpp — CPU check of the pair form of the degree-4 constraint sum (boundless_amd/csrc/circuit_dev.hpp): the plan
// PairPlan<TT> itself (every term once, each term's two pairs multiply to exactly its four pool entries, no group with a pair in
// common, no group beyond GRP terms, every pair computed at or before each of its uses, the pairs really distinct) and the values of
// cons_sum<TT, 4> against the plain canonical loop cons_sum<0, 0>, for T = 64 (the dispatched shape) and for term counts that leave
// the groups uneven, down to a single term.  Compiled with -DBX_CHECK_BOUNDS, so every sredc operand, every pair product and every
// second- and third-level sum is asserted against its bound; the pools are those of cons_factored_check.cpp.
// Built and run by tests/test_cons_pairs_cpu.py; a stand-alone program, so it is also built with -fsanitize=undefined,address.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "fp.hpp"
#include "poseidon2_arith.hpp"
#include "circuit_dev.hpp"

using namespace bx;

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static const uint32_t HALF = P / 2, NHALF = P / 2 + 1;  // centred: +P/2 and -P/2
static const int RANDOM_POOLS = 120000;

#define FAIL(...)                                  \
    do {                                           \
        fprintf(stderr, "PairPlan<%d>: ", TT);     \
        fprintf(stderr, __VA_ARGS__);              \
        fprintf(stderr, "\n");                     \
        return 1;                                  \
    } while (0)

template <int TT>
static int check_plan() {
    const PairPlan<TT>& plan = pair_plan<TT>;
    constexpr int GRP = PairPlan<TT>::GRP;
    if (plan.np < 1 || plan.np > 2 * TT || plan.pbeg[0] != 0 || plan.pbeg[TT] != plan.np) FAIL("%d pairs, first uses end at %d", plan.np, plan.pbeg[TT]);
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
            // computed at this slot or an earlier one
            if (p < 0 || p >= plan.pbeg[s + 1]) FAIL("slot %d uses pair %d before it is computed (%d so far)", s, p, plan.pbeg[s + 1]);
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
        // its first use is the slot that computes it
        int s = 0;
        while (plan.pbeg[s + 1] <= p) ++s;
        if (plan.s1[s] != p && plan.s2[s] != p) FAIL("pair %d is computed at slot %d, which does not use it", p, s);
    }
    if (plan.ng < 1 || plan.gbeg[0] != 0 || plan.gbeg[plan.ng] != TT || plan.lbeg[0] != 0 || plan.lbeg[plan.n2] != plan.ng) FAIL("%d groups end at slot %d, %d second-level groups at group %d", plan.ng, plan.gbeg[plan.ng], plan.n2, plan.lbeg[plan.n2]);
    for (int g = 0; g < plan.ng; ++g) {
        const int b = plan.gbeg[g], e = plan.gbeg[g + 1];
        if (e <= b || e - b > GRP) FAIL("group %d holds %d terms", g, e - b);
        for (int s = b; s < e; ++s)
            for (int r = b; r < s; ++r)
                if (plan.s1[s] == plan.s1[r] || plan.s1[s] == plan.s2[r] || plan.s2[s] == plan.s1[r] || plan.s2[s] == plan.s2[r]) FAIL("group %d: slots %d and %d share a pair", g, r, s);
    }
    for (int l = 0; l < plan.n2; ++l)
        if (plan.lbeg[l + 1] <= plan.lbeg[l]) FAIL("second-level group %d is empty", l);
    printf("PairPlan<%d>: %d distinct pairs, %d groups, %d second-level groups, at most %d pairs alive\n", TT, plan.np, plan.ng, plan.n2, plan.max_live);
    if (TT == 64 && plan.np > 51) FAIL("%d distinct pairs, more than 51", plan.np);
    return 0;
}

template <int TT>
static int check_one(const uint32_t (&pool)[Circuit::POOL], const char* what, int iter) {
    const uint32_t want = cons_sum<0, 0>(pool, TT, 4), got = cons_sum<TT, 4>(pool, TT, 4);
    if (got != want || got >= P) {
        fprintf(stderr, "cons_sum<%d,4> mismatch on %s pool %d: got %u want %u\n", TT, what, iter, got, want);
        return 1;
    }
    return 0;
}

template <int TT>
static int check_shape() {
    if (check_plan<TT>()) return 1;
    uint32_t pool[Circuit::POOL];
    // all +P/2, all -P/2, alternating signs (both phases, and in runs of two and four)
    for (int mode = 0; mode < 8; ++mode) {
        for (unsigned i = 0; i < Circuit::POOL; ++i) {
            const unsigned bit = mode < 2 ? (unsigned)mode : mode < 4 ? (i + mode) & 1u : mode < 6 ? ((i >> 1) + mode) & 1u : ((i >> 2) + mode) & 1u;
            pool[i] = bit ? NHALF : HALF;
        }
        if (check_one<TT>(pool, "extreme", mode)) return 1;
    }
    // every entry +-P/2 with signs drawn at random: the accumulators' largest magnitudes come from sign patterns that align a group
    for (int iter = 0; iter < 40000; ++iter) {
        const uint64_t r = rnd64();
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = ((r >> i) & 1) ? NHALF : HALF;
        if (check_one<TT>(pool, "random-sign", iter)) return 1;
    }
    // edge words mixed with random ones
    const uint32_t edge[] = {0, 1, P - 1, HALF, NHALF, HALF - 1, MONT_ONE, P - MONT_ONE};
    for (int iter = 0; iter < 40000; ++iter) {
        for (unsigned i = 0; i < Circuit::POOL; ++i) {
            const uint64_t r = rnd64();
            pool[i] = (r & 1) ? edge[(r >> 8) % 8] : (uint32_t)((r >> 8) % P);
        }
        if (check_one<TT>(pool, "edge-mix", iter)) return 1;
    }
    for (int iter = 0; iter < RANDOM_POOLS; ++iter) {
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = (uint32_t)(rnd64() % P);
        if (check_one<TT>(pool, "random", iter)) return 1;
    }
    return 0;
}

int main() {
    if (check_shape<64>() || check_shape<33>() || check_shape<17>() || check_shape<7>() || check_shape<1>()) return 1;
    printf("cons_pairs_check ok\n");
    return 0;
}
