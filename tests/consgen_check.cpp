// consgen_check.cpp — stand-alone checker of the constraint-program emitter (csrc/cons_program_emit.cpp), built with
// -fsanitize=address,undefined by tests/test_consgen_cpu.py and run as a process of its own.
//
// Seeded descriptors of the generator family of tests/cons_program_check.cpp go through bx_cons_program_create; for every one that
// compiles:
//   bx_cons_program_emit_hip with a NULL buffer gives the size; with cap = need - 1 it is refused and writes NOTHING (the buffer is an
//   exact-size heap block between two guard patterns, and ASan watches its ends); with cap = need it writes need bytes, NUL last;
//   a second emit is byte-equal; the digest is stable, equals the one the text carries, and changes when one constant changes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
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

struct Case {
    std::vector<bx_cons_step> steps;
    std::vector<bx_cons_tap> taps;
    uint32_t n_globals = 0, ret = 0;
};

// well-formed by construction except for live-value pressure, which create may refuse (as in cons_program_check.cpp)
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

static bx_cons_program* create(const Case& c) {
    bx_cons_program_desc d{c.steps.data(), c.steps.size(), c.taps.data(), c.taps.size(), c.n_globals, c.ret};
    bx_cons_program* prog = nullptr;
    return bx_cons_program_create(&d, &prog) ? nullptr : prog;
}

#define FAIL(...)                      \
    do {                               \
        printf("seed %u: ", seed);     \
        printf(__VA_ARGS__);           \
        printf("\n");                  \
        return 1;                      \
    } while (0)

int main() {
    long emitted = 0, with_const = 0;
    size_t longest = 0;
    for (uint32_t seed = 0; seed < 3000; ++seed) {
        g_state = 0xC0115EEDull * (seed + 1);
        Case c = well_formed(seed % 7 == 0 ? 400 + below(600) : 3 + below(80), seed % 5 == 0 ? 25 : 2);
        bx_cons_program* prog = create(c);
        if (!prog) continue;  // live-value pressure: the compiler's refusals are cons_program_check.cpp's subject
        size_t need = 0, need2 = 0;
        if (const char* e = bx_cons_program_emit_hip(prog, nullptr, 0, &need)) FAIL("emit with a NULL buffer: %s", e);
        if (need < 100) FAIL("a text of %zu bytes", need);
        // cap = need - 1: refused, nothing written (an exact-size heap block: ASan reports a write past its end)
        {
            char* buf = (char*)malloc(need - 1);
            memset(buf, 0x5A, need - 1);
            const char* e = bx_cons_program_emit_hip(prog, buf, need - 1, &need2);
            if (!e || need2 != need) FAIL("a short buffer was not refused with the size (need %zu, got %zu)", need, need2);
            for (size_t k = 0; k + 1 < need; ++k)
                if (buf[k] != 0x5A) FAIL("a refused emit wrote byte %zu", k);
            free(buf);
        }
        std::string a(need, '\x5A'), b(need, '\x33');
        if (const char* e = bx_cons_program_emit_hip(prog, &a[0], need, &need2)) FAIL("emit with cap = need: %s", e);
        if (need2 != need || a[need - 1] != '\0' || strlen(a.c_str()) != need - 1) FAIL("the text is not need - 1 characters and a NUL");
        if (const char* e = bx_cons_program_emit_hip(prog, &b[0], need, &need2)) FAIL("second emit: %s", e);
        if (a != b) FAIL("two emits of one program differ");
        // a larger buffer: nothing past need
        {
            std::string big(need + 64, '\x77');
            if (const char* e = bx_cons_program_emit_hip(prog, &big[0], big.size(), &need2)) FAIL("emit into a larger buffer: %s", e);
            for (size_t k = need; k < big.size(); ++k)
                if (big[k] != '\x77') FAIL("emit wrote past the text, at byte %zu", k);
        }
        uint32_t d1[8], d2[8];
        if (bx_cons_program_digest(prog, d1) || bx_cons_program_digest(prog, d2) || memcmp(d1, d2, 32) != 0) FAIL("the digest is not stable");
        char first[16];
        snprintf(first, sizeof first, "0x%08xu", d1[0]);
        if (a.find(first) == std::string::npos) FAIL("the text does not carry the digest");
        // the same descriptor compiled again: same digest, same text
        bx_cons_program* again = create(c);
        if (!again || bx_cons_program_digest(again, d2) || memcmp(d1, d2, 32) != 0) FAIL("the same description gave another digest");
        bx_cons_program_destroy(again);
        // one constant changed
        for (bx_cons_step& s : c.steps)
            if (s.op == BX_CONS_CONST || s.op == BX_CONS_CONST_EXT) {
                s.a = (s.a + 1) % P;
                bx_cons_program* other = create(c);
                if (!other || bx_cons_program_digest(other, d2)) FAIL("the changed description does not compile");
                if (memcmp(d1, d2, 32) == 0) FAIL("one constant changed and the digest did not");
                bx_cons_program_destroy(other);
                ++with_const;
                break;
            }
        longest = need > longest ? need : longest;
        ++emitted;
        bx_cons_program_destroy(prog);
    }
    printf("emitted %ld programs (%ld with a constant changed), longest text %zu bytes\n", emitted, with_const, longest);
    if (emitted < 500 || with_const < 300) {
        printf("the case mix is too thin to mean anything\n");
        return 1;
    }
    printf("consgen_check ok\n");
    return 0;
}
