// cons_levels_check.cpp — CPU check of the centred entry point of the constraint sum (boundless_amd/csrc/circuit_dev.hpp): the
// overload cons_sum<TT, GG>(const i32 (&)[POOL], T, G) that witness_derive_kernel and eval_check_kernel call with the pool their
// DerivedRegs<true> keep centred from one cell to the next, against the plain canonical loop cons_sum<0, 0> on the same pool as
// canonical words — and against the canonical-pool signature, which centres per call — for T = 64, 33, 17, 7, 1 at G = 4 and for
// (48, 3), (16, 3); and a walk of 19 derived cells (two runs of eight and three more: slot 1 is a back-tap at j = 0, 4, 8, 12, 16)
// through DerivedRegs<true> with entries centred where they are loaded or produced against the same walk through
// DerivedRegs<false> with canonical entries and the plain loop.  Compiled with -DBX_CHECK_BOUNDS by tests/test_cons_levels_cpu.py,
// so the magnitude of every entering pool entry (|c| <= P/2), every sredc operand and every level's sum is asserted on the way (run
// with the argument `uncentred` it hands over one entry of P/2 + 1, which that build must refuse); a stand-alone program, so it is
// also built with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
static const int RANDOM_POOLS = 4000, RANDOM_WALKS = 400, WALK = 19;

// fill `pool`: modes 0..4 are the fixed pools (all P/2, all P/2 + 1, alternating, 0, P - 1), anything else is random
static void make_words(uint32_t* w, int n, int mode) {
    for (int i = 0; i < n; ++i)
        w[i] = mode == 0 ? HALF : mode == 1 ? NHALF : mode == 2 ? ((i & 1) ? NHALF : HALF) : mode == 3 ? 0u : mode == 4 ? P - 1 : (uint32_t)(rnd64() % P);
}

template <int TT, int GG>
static int check_pool(const uint32_t (&pool_u)[Circuit::POOL], int mode, int iter) {
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
        fprintf(stderr, "cons_sum<%d,%d> mismatch on pool mode %d iteration %d: centred entry %u, canonical entry %u, plain loop %u\n", TT, GG, mode, iter,
                got, canon, want);
        return 1;
    }
    return 0;
}

template <int TT, int GG>
static int check_shape() {
    uint32_t pool[Circuit::POOL];
    for (int mode = 0; mode < 5; ++mode) {
        make_words(pool, Circuit::POOL, mode);
        if (check_pool<TT, GG>(pool, mode, 0)) return 1;
    }
    for (int iter = 0; iter < RANDOM_POOLS; ++iter) {
        make_words(pool, Circuit::POOL, 5);
        if (check_pool<TT, GG>(pool, 5, iter)) return 1;
    }
    return 0;
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
    make_words(row.back, WALK, mode == 2 ? 2 : mode);
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
    if (check_shape<64, 4>() || check_shape<33, 4>() || check_shape<17, 4>() || check_shape<7, 4>() || check_shape<1, 4>() || check_shape<48, 3>() ||
        check_shape<16, 3>())
        return 1;
    for (int c = 0; c < 2; ++c) {
        for (int mode = 0; mode < 5; ++mode)
            if (check_walk(mode, 0, c != 0)) return 1;
        for (int iter = 0; iter < RANDOM_WALKS; ++iter)
            if (check_walk(5, iter, c != 0)) return 1;
    }
    printf("cons_levels_check ok\n");
    return 0;
}
