// ext_mix_check.cpp — CPU check of the weighted ext accumulator and of the tail of the synthetic circuit's eval_check
// (boundless_amd/csrc/lazy_ext.hpp: WeightedExtAcc, accumulator_value, pair_value, and LazyExtAcc for the base-valued constraints)
// against the canonical composition of fp.hpp (f4_mul, f4_scale, f4_add, f4_sub), component by component and canonical.
// Built by tests/test_ext_mix_cpu.py plainly, with -DBX_CHECK_BOUNDS (every fold operand, every chain after every term, the operand
// of every reduction and every value handed to the accumulator is asserted) and with the bounds under the address and
// undefined-behaviour sanitizers, where a chain that left 64 bits is a signed overflow.
//   ext_mix_check             all checks
//   ext_mix_check overweight  one term with a weight one step outside [-P/2, P/2]: refused where bounds are asserted
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fp.hpp"
#include "lazy_ext.hpp"

using namespace bx;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t rnd_word() { return (uint32_t)(rnd64() % P); }
static Fp4 rnd_elem() { return Fp4{{rnd_word(), rnd_word(), rnd_word(), rnd_word()}}; }
static uint32_t word_of(i32 v) { return (uint32_t)(((int64_t)v % (int64_t)P + (int64_t)P) % (int64_t)P); }  // any signed word -> canonical
static bool same(const Fp4& got, const Fp4& want) {
    for (int c = 0; c < 4; ++c)
        if (got.c[c] != want.c[c] || got.c[c] >= P) return false;
    return true;
}
#define REQUIRE(cond, ...)                                             \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "FAILED %s (line %d): ", #cond, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                              \
            fprintf(stderr, "\n");                                     \
            return 1;                                                  \
        }                                                              \
    } while (0)

// ---- WeightedExtAcc: sum_k W_k * V_k against f4_mul + f4_add ----
static int weighted_sum(int n, int wmode, int vmode) {
    // wmode 0..15: every weight +-P/2, bit c set -> component c is -P/2; 16: random
    // vmode 0: all +P/2, 1: all -P/2, 2: alternating by component, 3: alternating by term, 4: all +(P - 1), 5: all -(P - 1), 6: all +P,
    //       7: all -P (the value bound itself), 8: random canonical, 9: random in [-P, P]
    WeightedExtAcc acc;
    acc.reset();
    Fp4 want = f4_zero();
    for (int k = 0; k < n; ++k) {
        i32 w[4], v[4];
        for (int c = 0; c < 4; ++c) {
            w[c] = wmode < 16 ? (((wmode >> c) & 1) ? -(i32)(P / 2) : (i32)(P / 2)) : fp_centre(rnd_word());
            const i32 h = (i32)(P / 2), f = (i32)(P - 1);
            switch (vmode) {
                case 0: v[c] = h; break;
                case 1: v[c] = -h; break;
                case 2: v[c] = (c & 1) ? -h : h; break;
                case 3: v[c] = (k & 1) ? -h : h; break;
                case 4: v[c] = f; break;
                case 5: v[c] = -f; break;
                case 6: v[c] = (i32)P; break;
                case 7: v[c] = -(i32)P; break;
                case 8: v[c] = (i32)rnd_word(); break;
                default: v[c] = (i32)((int64_t)(rnd64() % (2ull * P + 1)) - (int64_t)P); break;
            }
        }
        acc.add(w, v);
        want = f4_add(want, f4_mul(Fp4{{word_of(w[0]), word_of(w[1]), word_of(w[2]), word_of(w[3])}}, Fp4{{word_of(v[0]), word_of(v[1]), word_of(v[2]), word_of(v[3])}}));
    }
    const Fp4 got = acc.finish();
    REQUIRE(same(got, want), "WeightedExtAcc: %d terms, weights %d, values %d", n, wmode, vmode);
    return 0;
}
static int check_weighted_acc() {
    // folds come after every term (coefficients 2, 3, 4), every second (1, 5) and every fourth (0, 6): every count up to 40 lies within one
    // of each boundary, and a long run follows
    std::vector<int> counts;
    for (int n = 0; n <= 40; ++n) counts.push_back(n);
    counts.push_back(1000);
    for (int n : counts)
        for (int wmode = 0; wmode <= 16; ++wmode)
            for (int vmode = 0; vmode < 10; ++vmode)
                if (weighted_sum(n, wmode, vmode)) return 1;
    return 0;
}

// ---- the tail of eval_check_kernel: the new form as circuit.hip composes it, and the canonical form it replaced ----
struct Tail {
    uint32_t J, E, pairs, globals;
    uint32_t first, last, g[2], d0, dlast;
    std::vector<uint32_t> cons;             // J base-valued constraints (the walk's)
    std::vector<Fp4> a, ab, beta, hi, lo;   // accumulator e: its column at the point and one row back, its challenge; pair p: the two columns
    std::vector<uint32_t> x;                // accumulator e's data word
    std::vector<Fp4> mix;                   // the mix powers (any ext elements do)
};
static Fp4 tail_canonical(const Tail& t) {
    Fp4 tot = f4_zero();
    for (uint32_t j = 0; j < t.J; ++j) tot = f4_add(tot, f4_scale(t.mix[j], t.cons[j]));
    for (uint32_t e = 0; e < t.E; ++e) {
        Fp4 inner = f4_scale(t.ab[e], fp_sub(MONT_ONE, t.first));
        inner.c[0] = fp_add(inner.c[0], t.first);
        const Fp4 fac{{fp_add(t.beta[e].c[0], t.x[e]), t.beta[e].c[1], t.beta[e].c[2], t.beta[e].c[3]}};
        tot = f4_add(tot, f4_mul(t.mix[t.J + e], f4_sub(t.a[e], f4_mul(inner, fac))));
    }
    for (uint32_t p = 0; p < t.pairs; ++p) {
        Fp4 d;
        for (int k = 0; k < 4; ++k) d.c[k] = fp_sub(t.hi[p].c[k], t.lo[p].c[k]);
        tot = f4_add(tot, f4_mul(t.mix[t.J + t.E + p], f4_scale(d, t.last)));
    }
    const size_t b0 = (size_t)t.J + t.E + t.pairs;
    tot = f4_add(tot, f4_scale(t.mix[b0], fp_mul(t.first, fp_sub(t.d0, t.g[0]))));
    if (t.globals > 1) tot = f4_add(tot, f4_scale(t.mix[b0 + 1], fp_mul(t.last, fp_sub(t.dlast, t.g[1]))));
    return tot;
}
static void centred(const Fp4& m, i32 w[4]) {
    for (int c = 0; c < 4; ++c) w[c] = fp_centre(m.c[c]);
}
static Fp4 tail_lazy(const Tail& t) {
    i32 w[4], v[4], beta[4];
    LazyExtAcc mixacc;
    mixacc.reset();
    for (uint32_t j = 0; j < t.J; ++j) {
        centred(t.mix[j], w);
        mixacc.add(w, t.cons[j]);
    }
    const size_t b0 = (size_t)t.J + t.E + t.pairs;
    centred(t.mix[b0], w);
    mixacc.add(w, fp_mul(t.first, fp_sub(t.d0, t.g[0])));
    if (t.globals > 1) {
        centred(t.mix[b0 + 1], w);
        mixacc.add(w, fp_mul(t.last, fp_sub(t.dlast, t.g[1])));
    }
    const Fp4 base = mixacc.finish();
    const TailSelectors sel = tail_selectors(t.first, t.last);
    WeightedExtAcc extacc;
    extacc.reset();
    for (uint32_t e = 0; e < t.E; ++e) {
        centred(t.beta[e], beta);
        accumulator_value(t.a[e], t.ab[e], sel, beta, t.x[e], v);
        centred(t.mix[t.J + e], w);
        extacc.add(w, v);
    }
    for (uint32_t p = 0; p < t.pairs; ++p) {
        pair_value(t.hi[p], t.lo[p], sel, v);
        centred(t.mix[t.J + t.E + p], w);
        extacc.add(w, v);
    }
    return f4_add(base, extacc.finish());
}
// fill: 0 random, 1 all P/2, 2 all P/2 + 1 (= -P/2), 3 alternating, 4 all P - 1, 5 all 0
static uint32_t fill_word(int fill, unsigned i) {
    switch (fill) {
        case 0: return rnd_word();
        case 1: return P / 2;
        case 2: return P / 2 + 1;
        case 3: return (i & 1) ? P / 2 + 1 : P / 2;
        case 4: return P - 1;
        default: return 0u;
    }
}
static Fp4 fill_elem(int fill, unsigned i) { return Fp4{{fill_word(fill, i), fill_word(fill, i + 1), fill_word(fill, i + 2), fill_word(fill, i + 3)}}; }
static Tail make_tail(uint32_t J, uint32_t E, uint32_t pairs, uint32_t globals, uint32_t first, uint32_t last, uint32_t xword, bool xrandom, int fill_cols,
                      int fill_beta, int fill_mix) {
    Tail t;
    t.J = J, t.E = E, t.pairs = pairs, t.globals = globals, t.first = first, t.last = last;
    t.g[0] = fill_word(fill_cols, 0), t.g[1] = fill_word(fill_cols == 0 ? 0 : 5, 0), t.d0 = fill_word(fill_cols, 1), t.dlast = fill_word(fill_cols, 0);
    for (uint32_t j = 0; j < J; ++j) t.cons.push_back(fill_word(fill_cols, j));
    for (uint32_t e = 0; e < E; ++e) {
        t.a.push_back(fill_elem(fill_cols, e));
        t.ab.push_back(fill_elem(fill_cols, e + (fill_cols == 3 ? 1 : 0)));
        t.beta.push_back(fill_elem(fill_beta, e));
        t.x.push_back(xrandom ? rnd_word() : xword);
    }
    for (uint32_t p = 0; p < pairs; ++p) {
        t.hi.push_back(fill_elem(fill_cols, p));
        t.lo.push_back(fill_elem(fill_cols == 1 ? 2 : fill_cols == 2 ? 1 : fill_cols, p + 1));  // +P/2 against -P/2: the largest difference
    }
    for (size_t k = 0; k < (size_t)J + E + pairs + globals; ++k) t.mix.push_back(fill_elem(fill_mix, (unsigned)k));
    return t;
}
static int check_one_tail(const Tail& t, const char* what) {
    const Fp4 want = tail_canonical(t), got = tail_lazy(t);
    REQUIRE(same(got, want), "%s: J %u E %u pairs %u globals %u first %u last %u: got {%u,%u,%u,%u} want {%u,%u,%u,%u}", what, t.J, t.E, t.pairs, t.globals,
            t.first, t.last, got.c[0], got.c[1], got.c[2], got.c[3], want.c[0], want.c[1], want.c[2], want.c[3]);
    return 0;
}
static int check_tail() {
    const uint32_t sels[] = {0u, 1u, P - 1u, MONT_ONE, P / 2, P / 2 + 1};
    const uint32_t xs[] = {0u, P - 1u, P / 2, P / 2 + 1};
    // every selector pair, every data word, every extreme fill of the columns, of the challenges and of the mix powers, at the benchmark's
    // counts (E = 16, pairs = 8), at E = 1 / pairs = 0, without `last` (one boundary constraint) and with no ext-valued term at all
    const uint32_t shapes[][4] = {{5, 16, 8, 2}, {3, 1, 0, 2}, {2, 2, 0, 1}, {4, 0, 0, 2}, {0, 3, 1, 2}};
    for (const auto& sh : shapes)
        for (uint32_t first : sels)
            for (uint32_t last : sels)
                for (uint32_t x : xs)
                    for (int fc = 1; fc <= 5; ++fc)
                        for (int fb = 1; fb <= 4; ++fb)
                            for (int fm = 1; fm <= 3; ++fm)
                                if (check_one_tail(make_tail(sh[0], sh[1], sh[2], sh[3], first, last, x, false, fc, fb, fm), "extreme tail")) return 1;
    // term counts: every E and every number of pairs behind it up to 40 terms together, and a long run
    for (uint32_t E = 0; E <= 40; ++E)
        for (uint32_t pairs = 0; E + pairs <= 40; pairs += (pairs < 3 ? 1 : 7))
            for (int fill = 0; fill <= 3; ++fill)
                if (check_one_tail(make_tail(2, E, pairs, 2, fill == 0 ? rnd_word() : P - 1u, fill == 0 ? rnd_word() : P / 2 + 1, P / 2 + 1, fill == 0, fill, fill, fill),
                                   "term counts"))
                    return 1;
    for (int fill = 0; fill <= 3; ++fill)
        if (check_one_tail(make_tail(7, 600, 400, 2, P / 2 + 1, P / 2, P - 1u, fill == 0, fill, fill, fill), "long tail")) return 1;
    // random tails at random counts
    for (int it = 0; it < 20000; ++it)
        if (check_one_tail(make_tail((uint32_t)(rnd64() % 9), (uint32_t)(rnd64() % 18), (uint32_t)(rnd64() % 10), 1 + (uint32_t)(rnd64() & 1), rnd_word(), rnd_word(), 0,
                                     true, 0, 0, 0),
                           "random tail"))
            return 1;
    return 0;
}

// ---- a million random single constraints: the value words alone, and under one weight ----
static int check_random_terms() {
    const uint32_t sels[] = {0u, 1u, P - 1u, MONT_ONE};
    for (int it = 0; it < 1000000; ++it) {
        const bool edge = (it & 7) == 0;
        const uint32_t first = edge ? sels[rnd64() % 4] : rnd_word(), last = edge ? sels[rnd64() % 4] : rnd_word(), x = rnd_word();
        const Fp4 a = rnd_elem(), ab = rnd_elem(), beta = rnd_elem(), hi = rnd_elem(), lo = rnd_elem(), mixp = rnd_elem();
        const TailSelectors sel = tail_selectors(first, last);
        i32 bc[4], w[4], v[4];
        centred(beta, bc);
        centred(mixp, w);
        Fp4 inner = f4_scale(ab, fp_sub(MONT_ONE, first));
        inner.c[0] = fp_add(inner.c[0], first);
        const Fp4 want_a = f4_sub(a, f4_mul(inner, Fp4{{fp_add(beta.c[0], x), beta.c[1], beta.c[2], beta.c[3]}}));
        accumulator_value(a, ab, sel, bc, x, v);
        for (int c = 0; c < 4; ++c) REQUIRE(word_of(v[c]) == want_a.c[c] && v[c] <= (i32)P && v[c] >= -(i32)P, "accumulator_value, case %d component %d", it, c);
        WeightedExtAcc acc;
        acc.reset();
        acc.add(w, v);
        Fp4 want_p;
        for (int c = 0; c < 4; ++c) want_p.c[c] = fp_mul(fp_sub(hi.c[c], lo.c[c]), last);
        pair_value(hi, lo, sel, v);
        for (int c = 0; c < 4; ++c) REQUIRE(word_of(v[c]) == want_p.c[c] && v[c] <= (i32)P && v[c] >= -(i32)P, "pair_value, case %d component %d", it, c);
        acc.add(w, v);
        REQUIRE(same(acc.finish(), f4_add(f4_mul(mixp, want_a), f4_mul(mixp, want_p))), "two weighted constraints, case %d", it);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "overweight")) {
        WeightedExtAcc acc;
        acc.reset();
        const i32 w[4] = {(i32)(P / 2) + 1, 0, 0, 0}, v[4] = {1, 0, 0, 0};
        acc.add(w, v);
        const Fp4 r = acc.finish();
        printf("overweight accepted: %u\n", r.c[0]);
        return 0;
    }
    if (check_weighted_acc()) return 1;
    if (check_tail()) return 1;
    if (check_random_terms()) return 1;
    printf("ext_mix_check ok\n");
    return 0;
}
