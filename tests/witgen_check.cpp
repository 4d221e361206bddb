// witgen_check.cpp — stand-alone checker of the witness-program emitter (csrc/cons_program_emit.cpp), built with
// -fsanitize=address,undefined by tests/test_witgen_cpu.py and run as a process of its own.
//
// 3 000 seeded descriptors of the well-formed family of tests/wit_program_check.cpp go through bx_wit_program_create; for every one
// that compiles:
//   bx_wit_program_emit_hip with a NULL buffer gives the size; with cap = need - 1 it is refused and writes NOTHING (the buffer is an
//   exact-size heap block filled with a canary, and ASan watches its ends); with cap = need it writes need bytes, NUL last;
//   a second emit is byte-equal; the digest is stable, equals the one the text carries, changes when one constant, one tap or one SET
//   column changes, and does NOT change when only the global cells change.
// Then streams corrupted by hand (the compiled form is csrc/cons_program.hpp's): every one must be refused as "corrupt instruction
// stream"; and bx_cons_program_emit_hip must still refuse a constraint stream that holds a CP_ST.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "bx_program.h"
#include "cons_program.hpp"
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

constexpr uint32_t W_CODE = 3, W_DATA = 8;

struct Case {
    std::vector<bx_cons_step> steps;
    std::vector<bx_cons_tap> taps;
    std::vector<bx_wit_global_cell> cells;
    std::vector<uint32_t> free_cols, unused_cols;  // data columns that are not SET; of them, those no step names at all
};

// well-formed by the three derived-column rules, except for live-value pressure, which create may refuse (wit_program_check.cpp)
static Case well_formed(uint32_t n_steps, uint32_t far_share) {
    Case c;
    std::vector<uint32_t> derived, done;
    for (uint32_t col = 0; col < W_DATA; ++col) (col && below(2) ? derived : c.free_cols).push_back(col);  // column 0 is always free
    const auto tap = [&](uint32_t g, uint32_t col, uint32_t back) {
        c.taps.push_back(bx_cons_tap{g, col, back});
        return (uint32_t)c.taps.size() - 1;
    };
    uint32_t n_fp = 0;
    const auto pick = [&]() { return below(100) < far_share ? below(n_fp) : n_fp - 1 - below(n_fp < 6 ? n_fp : 6); };
    const uint32_t set_every = derived.empty() ? n_steps + 1 : (n_steps / (uint32_t)derived.size() > 2 ? n_steps / (uint32_t)derived.size() : 2);
    while (c.steps.size() < n_steps || done.size() < derived.size()) {
        if (done.size() < derived.size() && n_fp && c.steps.size() % set_every == set_every - 1) {
            c.steps.push_back(bx_cons_step{BX_CONS_SET, derived[done.size()], pick(), 0, 0});
            done.push_back(derived[done.size()]);
            continue;
        }
        const uint32_t k = below(100);
        if (n_fp < 2 || k < 30) {
            const uint32_t leaf = below(10);
            if (leaf < 1) c.steps.push_back(bx_cons_step{BX_CONS_CONST, below(P), 0, 0, 0});
            else if (leaf < 4) c.steps.push_back(bx_cons_step{BX_CONS_GET, tap(0, below(W_CODE), below(5)), 0, 0, 0});
            else if (leaf < 7 && !done.empty()) c.steps.push_back(bx_cons_step{BX_CONS_GET, tap(1, done[below((uint32_t)done.size())], 0), 0, 0, 0});
            else c.steps.push_back(bx_cons_step{BX_CONS_GET, tap(1, c.free_cols[below((uint32_t)c.free_cols.size())], below(5)), 0, 0, 0});
        } else {
            const uint32_t r = below(3);
            c.steps.push_back(bx_cons_step{r == 0 ? BX_CONS_ADD : (r == 1 ? BX_CONS_SUB : BX_CONS_MUL), pick(), pick(), 0, 0});
        }
        ++n_fp;
    }
    for (uint32_t g = 0, n = below(3); g < n; ++g) c.cells.push_back(bx_wit_global_cell{g, below(W_DATA), below(2)});
    for (uint32_t col : c.free_cols) {
        bool named = false;
        for (const bx_cons_tap& t : c.taps) named |= t.group == 1 && t.col == col;
        if (!named) c.unused_cols.push_back(col);
    }
    return c;
}

static bx_wit_program* create(const Case& c) {
    bx_wit_program_desc d{c.steps.data(), c.steps.size(), c.taps.data(), c.taps.size(), c.cells.data(), c.cells.size()};
    bx_wit_program* prog = nullptr;
    return bx_wit_program_create(&d, &prog) ? nullptr : prog;
}

// 1: `changed` compiles and has another digest than d1; 0: the same digest; -1: it does not compile
static int other_digest(const Case& changed, const uint32_t d1[8]) {
    bx_wit_program* other = create(changed);
    uint32_t d2[8];
    if (!other || bx_wit_program_digest(other, d2)) {
        bx_wit_program_destroy(other);
        return -1;
    }
    bx_wit_program_destroy(other);
    return memcmp(d1, d2, 32) != 0;
}

#define FAIL(...)                      \
    do {                               \
        printf("seed %u: ", seed);     \
        printf(__VA_ARGS__);           \
        printf("\n");                  \
        return 1;                      \
    } while (0)

static bool refused_as_corrupt(const bx_wit_program* prog, const char* what) {
    size_t need = 77;
    const char* e = bx_wit_program_emit_hip(prog, nullptr, 0, &need);
    if (e && strstr(e, "corrupt instruction stream") && need == 0) return true;
    printf("a stream with %s was not refused as corrupt (%s)\n", what, e ? e : "accepted");
    return false;
}

static int corrupt_streams() {
    // x = data[0](r-1) * code[1]; data[3] = x + 5
    const bx_cons_step steps[] = {{BX_CONS_GET, 0, 0, 0, 0}, {BX_CONS_GET, 1, 0, 0, 0}, {BX_CONS_MUL, 0, 1, 0, 0}, {BX_CONS_CONST, 5, 0, 0, 0},
                                  {BX_CONS_ADD, 2, 3, 0, 0}, {BX_CONS_SET, 3, 4, 0, 0}};
    const bx_cons_tap taps[] = {{1, 0, 1}, {0, 1, 0}};
    bx_wit_program_desc d{steps, 6, taps, 2, nullptr, 0};
    bx_wit_program* prog = nullptr;
    if (const char* e = bx_wit_program_create(&d, &prog)) return printf("corrupt_streams: create: %s\n", e), 1;
    size_t need = 0;
    if (const char* e = bx_wit_program_emit_hip(prog, nullptr, 0, &need)) return printf("corrupt_streams: the intact stream: %s\n", e), 1;
    const std::vector<uint32_t> code = prog->code;
    const std::vector<bx_cons_tap> tap_list = prog->taps;
    size_t at_tap = code.size(), at_mul = code.size(), at_ld = code.size(), at_st = code.size();
    for (size_t pc = 0; pc < code.size(); pc += 2) {
        const uint32_t op = code[pc] & 0xFFu;
        if (op == CP_TAP && at_tap == code.size()) at_tap = pc;
        if (op == CP_MUL_BB) at_mul = pc;
        if (op == CP_LD_B) at_ld = pc;
        if (op == CP_ST) at_st = pc;
    }
    if (at_tap == code.size() || at_mul == code.size() || at_ld == code.size() || at_st == code.size()) return printf("corrupt_streams: the stream lacks an opcode\n"), 1;
    const uint32_t nn = prog->info.narrow;
    bool ok = true;
    const auto with = [&](size_t pc, uint32_t w0, uint32_t w1, const char* what) {
        prog->code = code;
        prog->code[pc] = w0, prog->code[pc + 1] = w1;
        ok = refused_as_corrupt(prog, what) && ok;
        prog->code = code;
    };
    with(at_mul, cp_w0(CP_OPCODES, 0, 0, 0), 0, "an opcode >= CP_OPCODES");
    with(at_mul, cp_w0(0xFF, 0, 0, 0), 0, "opcode 255");
    with(at_mul, cp_w0(CP_MUL_EE, 0, 0, 0), 0, "a wide opcode (CP_MUL_EE)");
    with(at_mul, cp_w0(CP_ZERO, 0, 0, 0), 0, "a wide opcode (CP_ZERO)");
    with(at_mul, cp_w0(CP_LD_E, 0, 0, 0), 0, "a wide opcode (CP_LD_E)");
    with(at_mul, cp_w0(CP_MUL_BB, nn, 0, 0), 0, "a destination slot >= narrow");
    with(at_mul, cp_w0(CP_MUL_BB, 0, nn, 0), 0, "a source slot >= narrow");
    with(at_mul, cp_w0(CP_MUL_BB, 0, 0, 255), 0, "a source slot of 255");
    with(at_st, cp_w0(CP_ST, 0, nn, 0), code[at_st + 1], "a stored slot >= narrow");
    with(at_st, code[at_st], cp_w1(0, 4), "a store to a column above the largest SET column");
    with(at_tap, code[at_tap], cp_w1(0, (uint32_t)tap_list.size()), "a tap index past the table");
    with(at_tap, cp_w0(CP_TAP, nn, 0, 0), code[at_tap + 1], "a tap into a slot >= narrow");
    with(at_ld, code[at_ld], cp_w1(0, (uint32_t)prog->consts.size()), "a constant index past the table");
    prog->taps[0].group = 2;
    ok = refused_as_corrupt(prog, "tap group 2") && ok;
    prog->taps = tap_list;
    prog->code.push_back(0);  // an odd number of words
    ok = refused_as_corrupt(prog, "half an instruction") && ok;
    prog->code = code;
    if (const char* e = bx_wit_program_emit_hip(prog, nullptr, 0, &need)) return printf("corrupt_streams: the restored stream: %s\n", e), 1;
    bx_wit_program_destroy(prog);

    // a constraint stream with a store in it
    const bx_cons_step csteps[] = {{BX_CONS_GET, 0, 0, 0, 0}, {BX_CONS_TRUE, 0, 0, 0, 0}, {BX_CONS_AND_EQZ, 0, 0, 0, 0}};
    const bx_cons_tap ctaps[] = {{1, 0, 0}};
    bx_cons_program_desc cd{csteps, 3, ctaps, 1, 0, 1};
    bx_cons_program* cons = nullptr;
    if (const char* e = bx_cons_program_create(&cd, &cons)) return printf("corrupt_streams: cons create: %s\n", e), 1;
    if (const char* e = bx_cons_program_emit_hip(cons, nullptr, 0, &need)) return printf("corrupt_streams: the intact constraint stream: %s\n", e), 1;
    cons->code.push_back(cp_w0(CP_ST, 0, 0, 0));
    cons->code.push_back(cp_w1(0, 0));
    const char* e = bx_cons_program_emit_hip(cons, nullptr, 0, &need);
    if (!e || !strstr(e, "corrupt instruction stream")) {
        printf("bx_cons_program_emit_hip took a stream with a CP_ST (%s)\n", e ? e : "accepted");
        ok = false;
    }
    bx_cons_program_destroy(cons);
    return ok ? 0 : 1;
}

int main() {
    long emitted = 0, with_const = 0, with_tap = 0, with_set = 0, with_cells = 0;
    size_t longest = 0;
    for (uint32_t seed = 0; seed < 3000; ++seed) {
        g_state = 0x5E7C0DEull * (seed + 1);
        Case c = well_formed(seed % 7 == 0 ? 400 + below(600) : 3 + below(80), seed % 5 == 0 ? 25 : 2);
        bx_wit_program* prog = create(c);
        if (!prog) continue;  // live-value pressure: the compiler's refusals are wit_program_check.cpp's subject
        size_t need = 0, need2 = 0;
        if (const char* e = bx_wit_program_emit_hip(prog, nullptr, 0, &need)) FAIL("emit with a NULL buffer: %s", e);
        if (need < 100) FAIL("a text of %zu bytes", need);
        {
            char* buf = (char*)malloc(need - 1);
            memset(buf, 0x5A, need - 1);
            const char* e = bx_wit_program_emit_hip(prog, buf, need - 1, &need2);
            if (!e || need2 != need) FAIL("a short buffer was not refused with the size (need %zu, got %zu)", need, need2);
            for (size_t k = 0; k + 1 < need; ++k)
                if (buf[k] != 0x5A) FAIL("a refused emit wrote byte %zu", k);
            free(buf);
        }
        std::string a(need, '\x5A'), b(need, '\x33');
        if (const char* e = bx_wit_program_emit_hip(prog, &a[0], need, &need2)) FAIL("emit with cap = need: %s", e);
        if (need2 != need || a[need - 1] != '\0' || strlen(a.c_str()) != need - 1) FAIL("the text is not need - 1 characters and a NUL");
        if (const char* e = bx_wit_program_emit_hip(prog, &b[0], need, &need2)) FAIL("second emit: %s", e);
        if (a != b) FAIL("two emits of one program differ");
        {
            std::string big(need + 64, '\x77');
            if (const char* e = bx_wit_program_emit_hip(prog, &big[0], big.size(), &need2)) FAIL("emit into a larger buffer: %s", e);
            for (size_t k = need; k < big.size(); ++k)
                if (big[k] != '\x77') FAIL("emit wrote past the text, at byte %zu", k);
        }
        uint32_t d1[8], d2[8];
        if (bx_wit_program_digest(prog, d1) || bx_wit_program_digest(prog, d2) || memcmp(d1, d2, 32) != 0) FAIL("the digest is not stable");
        char first[16];
        snprintf(first, sizeof first, "0x%08xu", d1[0]);
        if (a.find(first) == std::string::npos) FAIL("the text does not carry the digest");
        if (other_digest(c, d1) != 0) FAIL("the same description gave another digest");
        // one constant changed
        for (size_t i = 0; i < c.steps.size(); ++i)
            if (c.steps[i].op == BX_CONS_CONST) {
                Case o = c;
                o.steps[i].a = (o.steps[i].a + 1) % P;
                if (other_digest(o, d1) != 1) FAIL("one constant changed and the digest did not");
                ++with_const;
                break;
            }
        // one tap changed: a code tap one row further back (no rule speaks about code columns)
        for (size_t k = 0; k < c.taps.size(); ++k)
            if (c.taps[k].group == 0) {
                Case o = c;
                o.taps[k].back += 1;
                if (other_digest(o, d1) != 1) FAIL("one tap changed and the digest did not");
                ++with_tap;
                break;
            }
        // one SET column changed: to a data column that no step names
        if (!c.unused_cols.empty())
            for (size_t i = 0; i < c.steps.size(); ++i)
                if (c.steps[i].op == BX_CONS_SET) {
                    Case o = c;
                    const uint32_t was = o.steps[i].a;
                    o.steps[i].a = c.unused_cols[0];
                    bool forwarded = false;  // a forwarded GET of the column would now be a load of a free one: another stream, not this check
                    for (const bx_cons_tap& t : c.taps) forwarded |= t.group == 1 && t.col == was;
                    if (forwarded) continue;
                    if (other_digest(o, d1) != 1) FAIL("one SET column changed and the digest did not");
                    ++with_set;
                    break;
                }
        // only the cells changed: the same digest, the same text
        {
            Case o = c;
            o.cells.clear();
            o.cells.push_back(bx_wit_global_cell{7, 0, 1});
            o.cells.push_back(bx_wit_global_cell{2, below(W_DATA), 0});
            bx_wit_program* other = create(o);
            if (!other || bx_wit_program_digest(other, d2)) FAIL("the description with other cells does not compile");
            if (memcmp(d1, d2, 32) != 0) FAIL("only the cells changed and the digest did too");
            std::string t2(need, '\0');
            if (bx_wit_program_emit_hip(other, &t2[0], need, &need2) || t2 != a) FAIL("only the cells changed and the text did too");
            bx_wit_program_destroy(other);
            ++with_cells;
        }
        longest = need > longest ? need : longest;
        ++emitted;
        bx_wit_program_destroy(prog);
    }
    printf("emitted %ld programs (changed: %ld constants, %ld taps, %ld SET columns, %ld cell lists), longest text %zu bytes\n", emitted, with_const, with_tap, with_set,
           with_cells, longest);
    if (emitted < 500 || with_const < 300 || with_tap < 300 || with_set < 100 || with_cells < 500) {
        printf("the case mix is too thin to mean anything\n");
        return 1;
    }
    if (corrupt_streams()) return 1;
    printf("witgen_check ok\n");
    return 0;
}
