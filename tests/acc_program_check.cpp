// acc_program_check.cpp — stand-alone checker of the accumulate-program compiler and host executor (csrc/program_compile.cpp, csrc/cons_program_host.cpp), built
// with -fsanitize=address,undefined by tests/test_acc_program_cpu.py and run as a process of its own.
//
// Seeded descriptors, well-formed and malformed, go through bx_acc_program_create.  Every one is either refused (with a message) or
// compiled; every compiled stream, run by bx_acc_program_run_host at po2 1, 3 and 6 over random and extreme columns and mixes, must
// agree with a DIRECT evaluation of the step list — every var a cell of its own, no slot file — written below and sharing only the
// field arithmetic of fp.hpp with the library.  That is the slot allocator's invariant: no live value is overwritten.  The direct
// evaluation also states the rules of the header itself and throws when create let a program through that breaks one.  Then every
// refusal of the header by its message, and the kept list: exactly the distinct tapped columns, in order of first appearance.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <stdexcept>
#include <utility>
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

constexpr uint32_t W_CODE = 3, W_DATA = 8, N_GLOBALS = 2, SPARE = 2;
constexpr uint32_t POISON = 0xDEADBEEFu;

struct Case {
    std::vector<bx_cons_step> steps;
    std::vector<bx_cons_tap> taps;
    uint32_t n_globals = N_GLOBALS;
};
struct Val {
    bool ext;
    Fp4 v;
};

// the header's table, literally, for one row: the term of every sequence (denominator and multiplicity, or factor)
struct Term {
    bool sum;
    Fp4 v;
    uint32_t m;
};
static std::map<uint32_t, Term> direct_row(const Case& c, uint32_t po2, uint32_t r, const std::vector<uint32_t>& code, const std::vector<uint32_t>& data,
                                           const uint32_t* globals, const uint32_t* mix) {
    const uint32_t n = 1u << po2;
    std::vector<Val> fp;
    std::map<uint32_t, Term> out;
    const auto base = [](uint32_t w) { return Val{false, Fp4{{w, 0u, 0u, 0u}}}; };
    for (const bx_cons_step& s : c.steps) {
        switch (s.op) {
        case BX_CONS_CONST: fp.push_back(base(fp_encode(s.a))); break;
        case BX_CONS_CONST_EXT: fp.push_back(Val{true, Fp4{{fp_encode(s.a), fp_encode(s.b), fp_encode(s.c), fp_encode(s.d)}}}); break;
        case BX_CONS_GET: {
            const bx_cons_tap& t = c.taps.at(s.a);
            if (t.group > 1) throw std::runtime_error("create accepted a tap of the accum group or beyond");
            fp.push_back(base((t.group == 0 ? code : data).at((size_t)t.col * n + ((r - t.back) & (n - 1u)))));
            break;
        }
        case BX_CONS_GET_GLOBAL:
            if (s.a > 1 || (s.a == 0 && s.b >= c.n_globals) || (s.a == 1 && s.b >= 4)) throw std::runtime_error("create accepted a GET_GLOBAL out of range");
            fp.push_back(base(s.a == 0 ? globals[s.b] : mix[s.b]));
            break;
        case BX_CONS_ADD: fp.push_back(Val{fp.at(s.a).ext || fp.at(s.b).ext, f4_add(fp.at(s.a).v, fp.at(s.b).v)}); break;
        case BX_CONS_SUB: fp.push_back(Val{fp.at(s.a).ext || fp.at(s.b).ext, f4_sub(fp.at(s.a).v, fp.at(s.b).v)}); break;
        case BX_CONS_MUL: fp.push_back(Val{fp.at(s.a).ext || fp.at(s.b).ext, f4_mul(fp.at(s.a).v, fp.at(s.b).v)}); break;
        case BX_CONS_SUM:
            if (fp.at(s.b).ext) throw std::runtime_error("create accepted an ext-typed m");
            if (!out.emplace(s.a, Term{true, fp.at(s.c).v, fp.at(s.b).v.c[0]}).second) throw std::runtime_error("create accepted a sequence defined twice");
            break;
        case BX_CONS_PROD:
            if (!out.emplace(s.a, Term{false, fp.at(s.b).v, 0u}).second) throw std::runtime_error("create accepted a sequence defined twice");
            break;
        default: throw std::runtime_error("create accepted an op that does not belong in an accumulate program");
        }
    }
    if (out.empty() || out.size() > BX_ACC_MAX_SEQS || out.rbegin()->first != out.size() - 1) throw std::runtime_error("create accepted S = 0, too many sequences or a gap");
    bool prod = false;
    for (const auto& kv : out) {
        if (kv.second.sum && prod) throw std::runtime_error("create accepted a PROD numbered below a SUM");
        prod |= !kv.second.sum;
    }
    return out;
}

// well-formed by construction except for live-value pressure, which create may refuse
static Case well_formed(uint32_t n_steps, uint32_t far_share) {
    Case c;
    const auto tap = [&](uint32_t g, uint32_t col, uint32_t back) {
        c.taps.push_back(bx_cons_tap{g, col, back});
        return (uint32_t)c.taps.size() - 1;
    };
    std::vector<bool> ext;
    const auto pick = [&]() {
        const uint32_t n_fp = (uint32_t)ext.size();
        return below(100) < far_share ? below(n_fp) : n_fp - 1 - below(n_fp < 6 ? n_fp : 6);
    };
    while (c.steps.size() < n_steps) {
        const uint32_t k = below(100);
        if (ext.size() < 2 || k < 30) {
            const uint32_t leaf = below(12);
            bool e = false;
            if (leaf < 1) c.steps.push_back(bx_cons_step{BX_CONS_CONST, below(P), 0, 0, 0});
            else if (leaf < 2) c.steps.push_back(bx_cons_step{BX_CONS_CONST_EXT, below(P), below(P), below(P), below(P)}), e = true;
            else if (leaf < 3) c.steps.push_back(bx_cons_step{BX_CONS_GET_GLOBAL, 0, below(N_GLOBALS), 0, 0});
            else if (leaf < 5) c.steps.push_back(bx_cons_step{BX_CONS_GET_GLOBAL, 1, below(4), 0, 0});
            else if (leaf < 8) c.steps.push_back(bx_cons_step{BX_CONS_GET, tap(0, below(W_CODE), below(5)), 0, 0, 0});
            else c.steps.push_back(bx_cons_step{BX_CONS_GET, tap(1, below(W_DATA), below(5)), 0, 0, 0});
            ext.push_back(e);
        } else {
            const uint32_t r = below(3), a = pick(), b = pick();
            c.steps.push_back(bx_cons_step{r == 0 ? BX_CONS_ADD : (r == 1 ? BX_CONS_SUB : BX_CONS_MUL), a, b, 0, 0});
            ext.push_back(ext[a] || ext[b]);
        }
    }
    const uint32_t sums = below(4), prods = below(3) + (sums ? 0 : 1);
    for (uint32_t s = 0; s < sums; ++s) {
        c.steps.push_back(bx_cons_step{BX_CONS_GET, tap(1, below(W_DATA), below(3)), 0, 0, 0});  // a base m
        ext.push_back(false);
        c.steps.push_back(bx_cons_step{BX_CONS_SUM, s, (uint32_t)ext.size() - 1, pick(), 0});
    }
    for (uint32_t s = sums; s < sums + prods; ++s) c.steps.push_back(bx_cons_step{BX_CONS_PROD, s, pick(), 0, 0});
    return c;
}
// a well-formed case with some fields overwritten by anything
static Case malformed() {
    Case c = well_formed(5 + below(60), 30);
    if (c.taps.empty()) c.taps.push_back(bx_cons_tap{1, 0, 0});
    const uint32_t hits = 1 + below(3);
    for (uint32_t h = 0; h < hits; ++h) {
        bx_cons_step& s = c.steps[below((uint32_t)c.steps.size())];
        switch (below(9)) {
        case 0: s.op = below(15); break;
        case 1: s.a = (uint32_t)rnd() >> below(32); break;
        case 2: s.b = (uint32_t)rnd() >> below(32); break;
        case 3: c.taps[below((uint32_t)c.taps.size())] = bx_cons_tap{below(4), below(W_DATA + 2), below(3)}; break;
        case 4: c.taps[below((uint32_t)c.taps.size())] = bx_cons_tap{below(5), (uint32_t)rnd() >> below(32), (uint32_t)rnd() >> below(32)}; break;
        case 5: s = bx_cons_step{BX_CONS_SUM, below(6), below(40), below(40), 0}; break;
        case 6: s = bx_cons_step{BX_CONS_PROD, below(6), below(40), 0, 0}; break;
        case 7: c.n_globals = below(70); break;
        default: s = bx_cons_step{below(14), below(40), below(40), below(40), (uint32_t)rnd()}; break;
        }
    }
    return c;
}

// columns and mixes: random, all 0, all P - 1, alternating 0 / P - 1
static void fill(std::vector<uint32_t>& v, uint32_t kind) {
    for (size_t i = 0; i < v.size(); ++i) v[i] = kind == 0 ? below(P) : (kind == 1 ? 0u : (kind == 2 ? P - 1 : (i & 1 ? P - 1 : 0u)));
}

static int fail(const char* what, const char* msg) {
    printf("%s: %s\n", what, msg ? msg : "(accepted)");
    return 1;
}

// every refusal of the header, by its message
static int refusals() {
    struct R {
        const char* want;
        std::vector<bx_cons_step> steps;
        std::vector<bx_cons_tap> taps;
        uint32_t n_globals;
    };
    const bx_cons_step one{BX_CONS_CONST, 1, 0, 0, 0}, ext{BX_CONS_CONST_EXT, 1, 2, 3, 4};
    std::vector<R> rs = {
        {"step 1: TRUE does not belong in an accumulate program", {one, {BX_CONS_TRUE, 0, 0, 0, 0}}, {}, 0},
        {"step 1: AND_EQZ does not belong in an accumulate program", {one, {BX_CONS_AND_EQZ, 0, 0, 0, 0}}, {}, 0},
        {"step 1: AND_COND does not belong in an accumulate program", {one, {BX_CONS_AND_COND, 0, 0, 0, 0}}, {}, 0},
        {"step 1: SET does not belong in an accumulate program", {one, {BX_CONS_SET, 0, 0, 0, 0}}, {}, 0},
        {"step 1: unknown op 13", {one, {13, 0, 0, 0, 0}}, {}, 0},
        {"tap 0: tap group 2 (accum): the program produces the accum group", {one, {BX_CONS_PROD, 0, 0, 0, 0}}, {{2, 0, 0}}, 0},
        {"tap group 3 out of range", {one}, {{3, 0, 0}}, 0},
        {"tap column 65536 out of range", {one}, {{0, 65536, 0}}, 0},
        {"tap back 65536 out of range", {one}, {{1, 0, 65536}}, 0},
        {"tap index 1 out of range", {{BX_CONS_GET, 1, 0, 0, 0}}, {{1, 0, 0}}, 0},
        {"SUM's m = 1 is ext-typed", {one, ext, {BX_CONS_SUM, 0, 1, 0, 0}}, {}, 0},
        {"step 2: sequence 0 is defined a second time (first at step 1)", {one, {BX_CONS_PROD, 0, 0, 0, 0}, {BX_CONS_SUM, 0, 0, 0, 0}}, {}, 0},
        {"sequence 1 is not defined: the sequences must be exactly 0 .. S-1", {one, {BX_CONS_PROD, 0, 0, 0, 0}, {BX_CONS_PROD, 2, 0, 0, 0}}, {}, 0},
        {"sequence 0 is not defined", {one, {BX_CONS_PROD, 1, 0, 0, 0}}, {}, 0},
        {"the program defines no sequence (S = 0)", {one}, {}, 0},
        {"sequence 1024 is not below BX_ACC_MAX_SEQS = 1024", {one, {BX_CONS_PROD, 1024, 0, 0, 0}}, {}, 0},
        {"SUM sequence 1 is numbered above a PROD sequence", {one, {BX_CONS_PROD, 0, 0, 0, 0}, {BX_CONS_SUM, 1, 0, 0, 0}}, {}, 0},
        {"constant 2013265921 is not below P", {{BX_CONS_CONST, P, 0, 0, 0}}, {}, 0},
        {"has a component not below P", {{BX_CONS_CONST_EXT, 0, 0, P, 0}}, {}, 0},
        {"operand b = 1 refers to a later or missing fp var", {one, {BX_CONS_ADD, 0, 1, 0, 0}}, {}, 0},
        {"operand d = 7 refers to a later or missing fp var", {one, {BX_CONS_SUM, 0, 0, 7, 0}}, {}, 0},
        {"operand a = 7 refers to a later or missing fp var", {one, {BX_CONS_PROD, 0, 7, 0, 0}}, {}, 0},
        {"global index 1 out of range (1 globals)", {{BX_CONS_GET_GLOBAL, 0, 1, 0, 0}}, {}, 1},
        {"mix component 4 out of range", {{BX_CONS_GET_GLOBAL, 1, 4, 0, 0}}, {}, 0},
        {"GET_GLOBAL table 2 out of range", {{BX_CONS_GET_GLOBAL, 2, 0, 0, 0}}, {}, 0},
        {"n_globals 65 is above BX_MAX_GLOBALS", {one}, {}, 65},
    };
    // live values: 33 base constants, then 25 ext ones, all named at the end
    for (int wide = 0; wide < 2; ++wide) {
        R r{wide ? "the program needs 25 live wide (ext) values, the limit is 24 (BX_CONS_MAX_WIDE)" : "the program needs 33 live narrow (base) values, the limit is 32 (BX_CONS_MAX_NARROW)",
            {}, {}, 0};
        const uint32_t n = wide ? 25 : 33;
        for (uint32_t k = 0; k < n; ++k) r.steps.push_back(wide ? ext : one);
        for (uint32_t k = 1; k < n; ++k) r.steps.push_back(bx_cons_step{BX_CONS_ADD, k == 1 ? 0 : n + k - 2, k, 0, 0});
        r.steps.push_back(bx_cons_step{BX_CONS_PROD, 0, 2 * n - 2, 0, 0});
        rs.push_back(r);
    }
    {
        R r{"steps, more than BX_CONS_MAX_STEPS", std::vector<bx_cons_step>(BX_CONS_MAX_STEPS + 1, one), {}, 0};
        rs.push_back(r);
        R t{"taps, more than BX_CONS_MAX_TAPS", {one}, std::vector<bx_cons_tap>(BX_CONS_MAX_TAPS + 1, bx_cons_tap{0, 0, 0}), 0};
        rs.push_back(t);
    }
    for (const R& r : rs) {
        bx_acc_program_desc d{r.steps.data(), r.steps.size(), r.taps.data(), r.taps.size(), r.n_globals};
        bx_acc_program* prog = nullptr;
        const char* msg = bx_acc_program_create(&d, &prog);
        if (!msg || prog || !strstr(msg, r.want) || strncmp(msg, "acc_program: ", 13)) {
            printf("wanted the refusal \"%s\", got: %s\n", r.want, msg ? msg : "(accepted)");
            bx_acc_program_destroy(prog);
            return 1;
        }
    }
    // the limits themselves compile: 32 narrow, 24 wide, sequence 1023
    {
        std::vector<bx_cons_step> steps{one};
        for (uint32_t s = 0; s < BX_ACC_MAX_SEQS; ++s) steps.push_back(bx_cons_step{BX_CONS_PROD, s, 0, 0, 0});
        bx_acc_program_desc d{steps.data(), steps.size(), nullptr, 0, 0};
        bx_acc_program* prog = nullptr;
        if (const char* msg = bx_acc_program_create(&d, &prog)) return fail("1024 sequences", msg);
        bx_acc_program_info info;
        bx_acc_program_info_get(prog, &info);
        bx_acc_program_destroy(prog);
        if (info.sequences != BX_ACC_MAX_SEQS || info.sums != 0 || info.narrow != 1 || info.wide != 0) return fail("1024 sequences", "info is wrong");
    }
    return 0;
}

int main() {
    if (refusals()) return 1;
    long compiled = 0, refused = 0, compiled_malformed = 0, ext_terms = 0;
    uint32_t peak_narrow = 0, peak_wide = 0;
    for (uint32_t seed = 0; seed < 3000; ++seed) {
        g_state = 0xACC0ull * (seed + 1);
        const bool bad = seed % 3 == 2;
        // short and long programs; mostly near operands (few live values: these compile), sometimes far ones (pressure: refusals)
        const Case c = bad ? malformed() : well_formed(seed % 7 == 0 ? 400 + below(600) : 3 + below(80), seed % 5 == 0 ? 25 : 2);
        bx_acc_program_desc d{c.steps.data(), c.steps.size(), c.taps.data(), c.taps.size(), c.n_globals};
        bx_acc_program* prog = nullptr;
        const char* msg = bx_acc_program_create(&d, &prog);
        if (msg) {
            if (prog || !*msg) return fail("a refusal left a program behind or has no message", msg);
            ++refused;
            continue;
        }
        if (!prog) return fail("neither refused nor compiled", nullptr);
        ++compiled;
        compiled_malformed += bad;
        bx_acc_program_info info;
        bx_acc_program_info_get(prog, &info);
        // kept: the distinct (group, col) of the tap list, in order of first appearance
        std::vector<std::pair<uint32_t, uint32_t>> kept;
        for (const bx_cons_tap& t : c.taps) {
            bool seen = false;
            for (const auto& k : kept) seen |= k.first == t.group && k.second == t.col;
            if (!seen) kept.emplace_back(t.group, t.col);
        }
        uint32_t S = 0, sums = 0;
        for (const bx_cons_step& s : c.steps) S += s.op == BX_CONS_SUM || s.op == BX_CONS_PROD, sums += s.op == BX_CONS_SUM;
        if (info.narrow > BX_CONS_MAX_NARROW || info.wide > BX_CONS_MAX_WIDE || info.steps != c.steps.size() || info.sequences != S || info.sums != sums ||
            info.instructions != c.steps.size() || info.taps != c.taps.size() || info.kept != kept.size() || info.n_globals != c.n_globals) {
            printf("seed %u: info is wrong (narrow %u, wide %u, steps %u, sequences %u, sums %u, instructions %u, kept %u)\n", seed, info.narrow, info.wide, info.steps,
                   info.sequences, info.sums, info.instructions, info.kept);
            return 1;
        }
        bool fits = true;
        for (uint32_t k = 0; k < info.kept; ++k) {
            uint32_t g = 9, col = 9;
            if (bx_acc_program_kept(prog, k, &g, &col) || g != kept[k].first || col != kept[k].second) {
                printf("seed %u: kept column %u is (%u, %u), the tap list says (%u, %u)\n", seed, k, g, col, kept[k].first, kept[k].second);
                return 1;
            }
            fits &= col < (g == 0 ? W_CODE : W_DATA);
        }
        uint32_t g9, c9;
        if (!bx_acc_program_kept(prog, info.kept, &g9, &c9)) return fail("kept took an index past the list", nullptr);
        peak_narrow = info.narrow > peak_narrow ? info.narrow : peak_narrow;
        peak_wide = info.wide > peak_wide ? info.wide : peak_wide;
        const uint32_t wa = 4 * S + SPARE;
        for (uint32_t po2 : {1u, 3u, 6u})
            for (uint32_t kind = 0; kind < 4; ++kind)
                for (uint32_t mkind = 0; mkind < 3; ++mkind) {
                    if ((po2 != 3 || mkind) && (kind || mkind) && seed % 4) continue;  // every column pattern at po2 3; the rest for a quarter of the seeds
                    const size_t n = (size_t)1 << po2;
                    std::vector<uint32_t> code(W_CODE * n), data(W_DATA * n), gm(64 + 4);
                    fill(code, kind);
                    fill(data, kind);
                    fill(gm, mkind);
                    const uint32_t *globals = gm.data(), *mix = gm.data() + 64;
                    std::vector<uint32_t> got(wa * n, POISON), want(wa * n, POISON);
                    const char* e = bx_acc_program_run_host(prog, po2, code.data(), W_CODE, data.data(), W_DATA, globals, mix, got.data(), wa);
                    if (!fits) {
                        if (!e || !*e || got != want) return fail("run_host took a program that taps a column beyond the widths, or wrote before it refused", e);
                        continue;
                    }
                    if (e) return fail("run_host", e);
                    try {
                        std::vector<Fp4> acc(S);
                        for (uint32_t r = 0; r < n; ++r) {
                            const std::map<uint32_t, Term> terms = direct_row(c, po2, r, code, data, globals, mix);
                            for (const auto& kv : terms) {
                                const uint32_t s = kv.first;
                                const Term& t = kv.second;
                                if (t.sum) {
                                    // 1 / d with 0 -> 0; d * x = 1 is CHECKED here, whatever produced x
                                    const Fp4 x = f4_is_zero(t.v) ? f4_zero() : f4_inv(t.v);
                                    if (!f4_is_zero(t.v)) {
                                        const Fp4 one = f4_mul(x, t.v);
                                        if (one.c[0] != MONT_ONE || one.c[1] || one.c[2] || one.c[3]) throw std::runtime_error("an inverse times its argument is not one");
                                    }
                                    acc[s] = f4_add(r ? acc[s] : f4_zero(), f4_scale(x, t.m));
                                    ext_terms += (t.v.c[1] | t.v.c[2] | t.v.c[3]) != 0;
                                } else {
                                    acc[s] = r ? f4_mul(acc[s], t.v) : t.v;
                                }
                                for (uint32_t k = 0; k < 4; ++k) want[(size_t)(4 * s + k) * n + r] = acc[s].c[k];
                            }
                        }
                    } catch (const std::exception& ex) {
                        printf("seed %u: create accepted a descriptor the definition cannot evaluate: %s\n", seed, ex.what());
                        return 1;
                    }
                    if (got != want) {
                        size_t k = 0;
                        while (got[k] == want[k]) ++k;
                        printf("seed %u po2 %u pattern %u mix %u: accum[%zu][%zu] is %u by the compiled stream, %u by the step list; %zu steps, narrow %u, wide %u\n", seed,
                               po2, kind, mkind, k / n, k % n, got[k], want[k], c.steps.size(), info.narrow, info.wide);
                        return 1;
                    }
                }
        bx_acc_program_destroy(prog);
    }
    printf("compiled %ld (of them malformed-but-valid %ld), refused %ld, ext denominators %ld, peak narrow %u, peak wide %u\n", compiled, compiled_malformed, refused,
           ext_terms, peak_narrow, peak_wide);
    if (compiled < 500 || refused < 300 || ext_terms < 500 || peak_narrow < 6 || peak_wide < 6) {
        printf("the case mix is too thin to mean anything\n");
        return 1;
    }
    printf("acc_program_check ok\n");
    return 0;
}
