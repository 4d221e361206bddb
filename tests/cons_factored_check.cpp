// cons_factored_check.cpp — CPU check of the factored constraint sum of boundless_amd/csrc/circuit_dev.hpp: cons_sum<TT, GG> against
// the plain canonical loop cons_sum<0, 0>, for every shape the library compiles (circuit.hip: BX_CIRCUIT_DISPATCH) and for shapes whose
// groups do not divide evenly (TT no multiple of 16) or whose chains are longer (GG = 5).  Compiled with -DBX_CHECK_BOUNDS, so every
// sredc operand on the way is asserted against SREDC_MAX; the pools are the worst cases of the centred arithmetic (all +P/2, all -P/2,
// alternating signs, every sign pattern of the 16 entries drawn at random), the edge words, and random words.
// Built and run by tests/test_cons_factored_cpu.py; a stand-alone program, so it can also be built with -fsanitize=undefined,address.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fp.hpp"
#include "poseidon2_arith.hpp"
#include "circuit_dev.hpp"

using namespace bx;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static const uint32_t HALF = P / 2, NHALF = P / 2 + 1;  // centred: +P/2 and -P/2
static const int RANDOM_POOLS = 120000;

template <int TT, int GG>
static int check_one(const uint32_t (&pool)[Circuit::POOL], const char* what, int iter) {
    const uint32_t want = cons_sum<0, 0>(pool, TT, GG), got = cons_sum<TT, GG>(pool, TT, GG);
    if (got != want || got >= P) {
        fprintf(stderr, "cons_sum<%d,%d> mismatch on %s pool %d: got %u want %u\n", TT, GG, what, iter, got, want);
        return 1;
    }
    return 0;
}

template <int TT, int GG>
static int check_shape() {
    uint32_t pool[Circuit::POOL];
    // the grouping itself: every term exactly once, under its own first factor
    if constexpr (GG >= 3) {
        const ConsPlan<TT, GG>& plan = cons_plan<TT, GG>;
        int seen[TT] = {0}, terms = 0;
        for (int q = 0; q < plan.nq; ++q)
            for (int k = 0; k < plan.len[q]; ++k) {
                const int t = plan.term[q][k];
                if (t < 0 || t >= TT || (int)Circuit::pool_idx((unsigned)t, 0u) != plan.first[q] || seen[t]++) {
                    fprintf(stderr, "ConsPlan<%d,%d>: inner group %d holds term %d wrongly\n", TT, GG, q, t);
                    return 1;
                }
                ++terms;
            }
        if (terms != TT || plan.obeg[plan.no] != plan.nq || plan.lbeg[plan.n2] != plan.no) {
            fprintf(stderr, "ConsPlan<%d,%d>: %d of %d terms grouped\n", TT, GG, terms, TT);
            return 1;
        }
    }
    // all +P/2, all -P/2, alternating signs (both phases, and in runs of two and four)
    for (int mode = 0; mode < 8; ++mode) {
        for (unsigned i = 0; i < Circuit::POOL; ++i) {
            const unsigned bit = mode < 2 ? (unsigned)mode : mode < 4 ? (i + mode) & 1u : mode < 6 ? ((i >> 1) + mode) & 1u : ((i >> 2) + mode) & 1u;
            pool[i] = bit ? NHALF : HALF;
        }
        if (check_one<TT, GG>(pool, "extreme", mode)) return 1;
    }
    // every entry +-P/2 with signs drawn at random: the accumulators' largest magnitudes come from sign patterns that align a group
    for (int iter = 0; iter < 40000; ++iter) {
        const uint64_t r = rnd64();
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = ((r >> i) & 1) ? NHALF : HALF;
        if (check_one<TT, GG>(pool, "random-sign", iter)) return 1;
    }
    // edge words mixed with random ones
    const uint32_t edge[] = {0, 1, P - 1, HALF, NHALF, HALF - 1, MONT_ONE, P - MONT_ONE};
    for (int iter = 0; iter < 40000; ++iter) {
        for (unsigned i = 0; i < Circuit::POOL; ++i) {
            const uint64_t r = rnd64();
            pool[i] = (r & 1) ? edge[(r >> 8) % 8] : (uint32_t)((r >> 8) % P);
        }
        if (check_one<TT, GG>(pool, "edge-mix", iter)) return 1;
    }
    for (int iter = 0; iter < RANDOM_POOLS; ++iter) {
        for (unsigned i = 0; i < Circuit::POOL; ++i) pool[i] = (uint32_t)(rnd64() % P);
        if (check_one<TT, GG>(pool, "random", iter)) return 1;
    }
    return 0;
}

int main() {
    // the dispatched shapes
    if (check_shape<64, 4>() || check_shape<48, 3>() || check_shape<16, 3>() || check_shape<8, 2>()) return 1;
    // longer chains, and term counts that leave the groups uneven
    if (check_shape<64, 5>() || check_shape<7, 4>() || check_shape<33, 3>() || check_shape<17, 4>()) return 1;
    printf("cons_factored_check ok\n");
    return 0;
}
