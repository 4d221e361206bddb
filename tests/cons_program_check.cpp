// cons_program_check.cpp — stand-alone checker of the constraint-program compiler and host executor (csrc/program_compile.cpp, csrc/cons_program_host.cpp), built
// with -fsanitize=address,undefined by tests/test_cons_program_check_cpu.py and run as a process of its own.
//
// Seeded descriptors, well-formed and malformed, go through bx_cons_program_create.  Every one is either refused (with a message) or
// compiled; every compiled stream, run by bx_cons_program_constraints_at, must agree with a DIRECT evaluation of the step list —
// unbounded var lists, mul computed, written below and sharing only the field arithmetic of fp.hpp with the library.  That is the
// slot allocator's invariant: no live value is overwritten.  Operands are drawn from anywhere in the lists, near and far, so that
// slots are freed, reused and held across long stretches.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <stdexcept>
#include <vector>

#include "bx_program.h"
#include "fp.hpp"

using namespace bx;

static uint64_t g_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return n ? (uint32_t)(rnd() % n) : 0u; }

static const char* tap_at(const void*, int group, uint32_t col, int back, uint32_t out[4]) {
    uint64_t s = ((uint64_t)group << 48) ^ ((uint64_t)col << 24) ^ (uint64_t)back;
    for (int k = 0; k < 4; ++k) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        out[k] = (uint32_t)((s >> 20) % P);
    }
    return nullptr;
}

struct Mix {
    Fp4 tot, mul;
};
// the header's table, literally; .at() throws if create let an operand through that names nothing
static Fp4 direct(const std::vector<bx_cons_step>& steps, const std::vector<bx_cons_tap>& taps, uint32_t ret, const Fp4& poly_mix, const uint32_t mixw[4],
                  const std::vector<uint32_t>& globals) {
    std::vector<Fp4> fp;
    std::vector<Mix> mx;
    for (const bx_cons_step& s : steps) {
        switch (s.op) {
        case BX_CONS_CONST: fp.push_back(Fp4{{fp_encode(s.a), 0u, 0u, 0u}}); break;
        case BX_CONS_CONST_EXT: fp.push_back(Fp4{{fp_encode(s.a), fp_encode(s.b), fp_encode(s.c), fp_encode(s.d)}}); break;
        case BX_CONS_GET: {
            const bx_cons_tap& t = taps.at(s.a);
            Fp4 v;
            tap_at(nullptr, (int)t.group, t.col, (int)t.back, v.c);
            fp.push_back(v);
            break;
        }
        case BX_CONS_GET_GLOBAL: fp.push_back(Fp4{{s.a == 0 ? globals.at(s.b) : mixw[s.b & 3u], 0u, 0u, 0u}}); break;
        case BX_CONS_ADD: fp.push_back(f4_add(fp.at(s.a), fp.at(s.b))); break;
        case BX_CONS_SUB: fp.push_back(f4_sub(fp.at(s.a), fp.at(s.b))); break;
        case BX_CONS_MUL: fp.push_back(f4_mul(fp.at(s.a), fp.at(s.b))); break;
        case BX_CONS_TRUE: mx.push_back(Mix{f4_zero(), f4_one()}); break;
        case BX_CONS_AND_EQZ: {
            const Mix x = mx.at(s.a);
            mx.push_back(Mix{f4_add(x.tot, f4_mul(x.mul, fp.at(s.b))), f4_mul(x.mul, poly_mix)});
            break;
        }
        case BX_CONS_AND_COND: {
            const Mix x = mx.at(s.a), in = mx.at(s.c);
            mx.push_back(Mix{f4_add(x.tot, f4_mul(f4_mul(fp.at(s.b), in.tot), x.mul)), f4_mul(x.mul, in.mul)});
            break;
        }
        default: throw std::runtime_error("create accepted an unknown op");
        }
    }
    return mx.at(ret).tot;
}

struct Case {
    std::vector<bx_cons_step> steps;
    std::vector<bx_cons_tap> taps;
    uint32_t n_globals = 0, ret = 0;
};

// well-formed by construction (degrees are tracked: a product that would pass 5 becomes a sum) except for live-value pressure, which
// create may refuse
static Case well_formed(uint32_t n_steps, uint32_t far_share) {
    Case c;
    c.n_globals = below(4);
    const uint32_t n_taps = 1 + below(20);
    for (uint32_t t = 0; t < n_taps; ++t) c.taps.push_back(bx_cons_tap{below(3), below(6), below(4)});
    uint32_t n_fp = 0, n_mix = 0;
    std::vector<uint32_t> fdeg, mdeg;
    const auto pick = [&](uint32_t n) { return below(100) < far_share ? below(n) : n - 1 - below(n < 6 ? n : 6); };
    while (c.steps.size() < n_steps) {
        bx_cons_step s{0, 0, 0, 0, 0};
        const uint32_t k = below(100);
        if (n_fp < 2 || k < 25) {
            const uint32_t leaf = below(10);
            if (leaf < 2) s = bx_cons_step{BX_CONS_CONST, below(P), 0, 0, 0};
            else if (leaf < 4) s = bx_cons_step{BX_CONS_CONST_EXT, below(P), below(P), below(P), below(P)};
            else if (leaf < 5) s = bx_cons_step{BX_CONS_GET_GLOBAL, 1, below(4), 0, 0};
            else if (leaf < 6 && c.n_globals) s = bx_cons_step{BX_CONS_GET_GLOBAL, 0, below(c.n_globals), 0, 0};
            else s = bx_cons_step{BX_CONS_GET, below(n_taps), 0, 0, 0};
            fdeg.push_back(s.op == BX_CONS_GET ? 1u : 0u);
            ++n_fp;
        } else if (k < 70) {
            const uint32_t r = below(10);
            s = bx_cons_step{r < 4 ? BX_CONS_ADD : (r < 7 ? BX_CONS_SUB : BX_CONS_MUL), pick(n_fp), pick(n_fp), 0, 0};
            if (s.op == BX_CONS_MUL && fdeg[s.a] + fdeg[s.b] > BX_CONS_MAX_DEGREE) s.op = BX_CONS_ADD;
            fdeg.push_back(s.op == BX_CONS_MUL ? fdeg[s.a] + fdeg[s.b] : (fdeg[s.a] > fdeg[s.b] ? fdeg[s.a] : fdeg[s.b]));
            ++n_fp;
        } else if (n_mix == 0 || k < 75) {
            s.op = BX_CONS_TRUE;
            mdeg.push_back(0u);
            ++n_mix;
        } else {
            s = bx_cons_step{BX_CONS_AND_COND, pick(n_mix), pick(n_fp), pick(n_mix), 0};
            if (k < 93 || fdeg[s.b] + mdeg[s.c] > BX_CONS_MAX_DEGREE) s.op = BX_CONS_AND_EQZ, s.c = 0;
            const uint32_t in = s.op == BX_CONS_AND_COND ? fdeg[s.b] + mdeg[s.c] : fdeg[s.b];
            mdeg.push_back(mdeg[s.a] > in ? mdeg[s.a] : in);
            ++n_mix;
        }
        c.steps.push_back(s);
    }
    if (!n_mix) c.steps.push_back(bx_cons_step{BX_CONS_TRUE, 0, 0, 0, 0}), ++n_mix;
    c.ret = below(100) < 80 ? n_mix - 1 : below(n_mix);
    return c;
}
// a well-formed case with some fields overwritten by anything
static Case malformed() {
    Case c = well_formed(5 + below(60), 30);
    const uint32_t hits = 1 + below(3);
    for (uint32_t h = 0; h < hits; ++h) {
        const uint32_t what = below(8);
        bx_cons_step& s = c.steps[below((uint32_t)c.steps.size())];
        switch (what) {
        case 0: s.op = below(14); break;
        case 1: s.a = (uint32_t)rnd(); break;
        case 2: s.b = (uint32_t)rnd(); break;
        case 3: s.c = (uint32_t)rnd(); break;
        case 4: c.ret = (uint32_t)rnd() >> below(32); break;
        case 5: c.taps[below((uint32_t)c.taps.size())] = bx_cons_tap{below(5), (uint32_t)rnd() >> below(32), (uint32_t)rnd() >> below(32)}; break;
        case 6: c.n_globals = below(70); break;
        default: s = bx_cons_step{below(11), below(40), below(40), below(40), (uint32_t)rnd()}; break;
        }
    }
    return c;
}

int main() {
    long compiled = 0, refused = 0, compiled_malformed = 0;
    uint32_t peak_narrow = 0, peak_wide = 0;
    for (uint32_t seed = 0; seed < 3000; ++seed) {
        g_state = 0xC0115EEDull * (seed + 1);
        const bool bad = seed % 3 == 2;
        // short and long programs; mostly near operands (few live values: these compile), sometimes far ones (pressure: refusals)
        const Case c = bad ? malformed() : well_formed(seed % 7 == 0 ? 400 + below(600) : 3 + below(80), seed % 5 == 0 ? 25 : 2);
        bx_cons_program_desc d{c.steps.data(), c.steps.size(), c.taps.data(), c.taps.size(), c.n_globals, c.ret};
        bx_cons_program* prog = nullptr;
        const char* msg = bx_cons_program_create(&d, &prog);
        if (msg) {
            if (prog || !*msg) {
                printf("seed %u: a refusal left a program behind or has no message\n", seed);
                return 1;
            }
            ++refused;
            continue;
        }
        if (!prog) {
            printf("seed %u: neither refused nor compiled\n", seed);
            return 1;
        }
        ++compiled;
        compiled_malformed += bad;
        bx_cons_program_info info;
        bx_cons_program_info_get(prog, &info);
        if (info.narrow > BX_CONS_MAX_NARROW || info.wide > BX_CONS_MAX_WIDE || info.degree > BX_CONS_MAX_DEGREE || info.steps != c.steps.size()) {
            printf("seed %u: info outside the limits (narrow %u wide %u degree %u)\n", seed, info.narrow, info.wide, info.degree);
            return 1;
        }
        peak_narrow = info.narrow > peak_narrow ? info.narrow : peak_narrow;
        peak_wide = info.wide > peak_wide ? info.wide : peak_wide;
        uint32_t pm[4], mixw[4], got[4];
        for (int k = 0; k < 4; ++k) pm[k] = below(P), mixw[k] = below(P);
        std::vector<uint32_t> globals(c.n_globals);
        for (uint32_t& g : globals) g = below(P);
        const bx_tap_reader reader{nullptr, tap_at};
        if (const char* e = bx_cons_program_constraints_at(prog, &reader, pm, mixw, globals.data(), got)) {
            printf("seed %u: constraints_at: %s\n", seed, e);
            return 1;
        }
        Fp4 want;
        try {
            want = direct(c.steps, c.taps, c.ret, Fp4{{pm[0], pm[1], pm[2], pm[3]}}, mixw, globals);
        } catch (const std::exception& e) {
            printf("seed %u: create accepted a descriptor the definition cannot evaluate: %s\n", seed, e.what());
            return 1;
        }
        if (memcmp(got, want.c, 16) != 0) {
            printf("seed %u: the compiled stream gives (%u %u %u %u), the step list (%u %u %u %u); %zu steps, narrow %u, wide %u\n", seed, got[0], got[1], got[2],
                   got[3], want.c[0], want.c[1], want.c[2], want.c[3], c.steps.size(), info.narrow, info.wide);
            return 1;
        }
        // taps: sorted, 0 first, within BX_MAX_TAPS
        for (const bx_cons_tap& t : c.taps) {
            uint32_t backs[BX_MAX_TAPS];
            const uint32_t n = bx_cons_program_taps(prog, (int)t.group, t.col, backs);
            bool has = false;
            for (uint32_t k = 0; k < n; ++k) has |= backs[k] == t.back;
            for (uint32_t k = 1; k < n; ++k) has &= backs[k - 1] < backs[k];
            if (!n || n > BX_MAX_TAPS || backs[0] != 0 || !has) {
                printf("seed %u: tap set of (%u, %u) is wrong\n", seed, t.group, t.col);
                return 1;
            }
        }
        bx_cons_program_destroy(prog);
    }
    printf("compiled %ld (of them malformed-but-valid %ld), refused %ld, peak narrow %u, peak wide %u\n", compiled, compiled_malformed, refused, peak_narrow, peak_wide);
    if (compiled < 500 || refused < 300 || peak_narrow < 8 || peak_wide < 8) {
        printf("the case mix is too thin to mean anything\n");
        return 1;
    }
    printf("cons_program_check ok\n");
    return 0;
}
