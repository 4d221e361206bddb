// acc_ratio_check.cpp — stand-alone checker of the RATIO step of accumulate programs in the compiler and the host executor
// (csrc/program_compile.cpp, csrc/cons_program_host.cpp), built with -fsanitize=address,undefined by tests/test_acc_ratio_cpu.py and run as a
// process of its own, in the manner of acc_program_check.cpp.
//
// 3 000 seeded descriptors with RATIO steps, well-formed and malformed, go through bx_acc_program_create.  Every one is either refused
// (with a message) or compiled; every compiled stream, run by bx_acc_program_run_host at po2 1, 3 and 6 over random, all-0, all-(P - 1)
// and alternating columns, must agree with a DIRECT evaluation of the step list — every var a cell of its own — that shares only the
// field arithmetic of fp.hpp with the library, with the columns at or above 4 S still poisoned.  The direct evaluation restates the
// rules (sums below products below ratios, each sequence once, no gap) and throws when create let a program through that breaks one.
// Then every new refusal by its text, and the op numbers that must stay unknown.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
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
enum Kind { SUM, PROD, RATIO };
struct Term {
    Kind kind;
    Fp4 v, den;  // denominator and multiplicity (SUM), factor (PROD), numerator and denominator (RATIO)
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
            if (!out.emplace(s.a, Term{SUM, fp.at(s.c).v, f4_zero(), fp.at(s.b).v.c[0]}).second) throw std::runtime_error("create accepted a sequence defined twice");
            break;
        case BX_CONS_PROD:
            if (!out.emplace(s.a, Term{PROD, fp.at(s.b).v, f4_zero(), 0u}).second) throw std::runtime_error("create accepted a sequence defined twice");
            break;
        case BX_CONS_RATIO:
            if (!out.emplace(s.a, Term{RATIO, fp.at(s.b).v, fp.at(s.c).v, 0u}).second) throw std::runtime_error("create accepted a sequence defined twice");
            break;
        default: throw std::runtime_error("create accepted an op that does not belong in an accumulate program");
        }
    }
    if (out.empty() || out.size() > BX_ACC_MAX_SEQS || out.rbegin()->first != out.size() - 1) throw std::runtime_error("create accepted S = 0, too many sequences or a gap");
    int top = SUM;
    for (const auto& kv : out) {  // in sequence order the kinds never go down
        if (kv.second.kind < top) throw std::runtime_error("create accepted sequences out of the order sums, products, ratios");
        top = kv.second.kind;
    }
    return out;
}

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
    // the NUMBERS are ordered, the defining steps are not: ratios first, then sums, then products, every other seed
    const uint32_t sums = below(3), prods = below(3), ratios = 1 + below(4);
    const bool ratios_first = below(2);
    const auto put_ratios = [&]() {
        for (uint32_t s = sums + prods; s < sums + prods + ratios; ++s) {
            const uint32_t a = pick(), b = pick();
            c.steps.push_back(bx_cons_step{BX_CONS_RATIO, s, a, b, 0});
        }
    };
    if (ratios_first) put_ratios();
    for (uint32_t s = 0; s < sums; ++s) {
        c.steps.push_back(bx_cons_step{BX_CONS_GET, tap(1, below(W_DATA), below(3)), 0, 0, 0});  // a base m
        ext.push_back(false);
        c.steps.push_back(bx_cons_step{BX_CONS_SUM, s, (uint32_t)ext.size() - 1, pick(), 0});
    }
    for (uint32_t s = sums; s < sums + prods; ++s) c.steps.push_back(bx_cons_step{BX_CONS_PROD, s, pick(), 0, 0});
    if (!ratios_first) put_ratios();
    return c;
}
static Case malformed() {
    Case c = well_formed(5 + below(60), 30);
    if (c.taps.empty()) c.taps.push_back(bx_cons_tap{1, 0, 0});
    const uint32_t hits = 1 + below(3);
    for (uint32_t h = 0; h < hits; ++h) {
        bx_cons_step& s = c.steps[below((uint32_t)c.steps.size())];
        switch (below(9)) {
        case 0: s.op = below(18); break;
        case 1: s.a = (uint32_t)rnd() >> below(32); break;
        case 2: s.b = (uint32_t)rnd() >> below(32); break;
        case 3: s.c = (uint32_t)rnd() >> below(32); break;
        case 4: c.taps[below((uint32_t)c.taps.size())] = bx_cons_tap{below(4), below(W_DATA + 2), below(3)}; break;
        case 5: s = bx_cons_step{BX_CONS_SUM, below(8), below(40), below(40), 0}; break;
        case 6: s = bx_cons_step{BX_CONS_PROD, below(8), below(40), 0, 0}; break;
        case 7: s = bx_cons_step{BX_CONS_RATIO, below(8), below(40), below(40), 0}; break;
        default: s = bx_cons_step{below(18), below(40), below(40), below(40), (uint32_t)rnd()}; break;
        }
    }
    return c;
}

static void fill(std::vector<uint32_t>& v, uint32_t kind) {
    for (size_t i = 0; i < v.size(); ++i) v[i] = kind == 0 ? below(P) : (kind == 1 ? 0u : (kind == 2 ? P - 1 : (i & 1 ? P - 1 : 0u)));
}

static int fail(const char* what, const char* msg) {
    printf("%s: %s\n", what, msg ? msg : "(accepted)");
    return 1;
}

static int refusals() {
    struct R {
        const char* who;
        const char* want;
        std::vector<bx_cons_step> steps;
    };
    const bx_cons_step one{BX_CONS_CONST, 1, 0, 0, 0};
    const std::vector<R> rs = {
        {"acc", "step 2: SUM sequence 1 is numbered above a RATIO sequence (step 1: RATIO sequence 0 is numbered below a SUM sequence)", {one, {BX_CONS_RATIO, 0, 0, 0, 0}, {BX_CONS_SUM, 1, 0, 0, 0}}},
        {"acc", "step 1: PROD sequence 1 is numbered above a RATIO sequence (step 2: RATIO sequence 0 is numbered below a PROD sequence): all sums come first, then all products, then all ratios",
         {one, {BX_CONS_PROD, 1, 0, 0, 0}, {BX_CONS_RATIO, 0, 0, 0, 0}}},
        {"acc", "SUM sequence 1 is numbered above a PROD sequence: all sums come first, then all products", {one, {BX_CONS_PROD, 0, 0, 0, 0}, {BX_CONS_SUM, 1, 0, 0, 0}, {BX_CONS_RATIO, 2, 0, 0, 0}}},
        {"acc", "step 2: sequence 0 is defined a second time (first at step 1)", {one, {BX_CONS_RATIO, 0, 0, 0, 0}, {BX_CONS_PROD, 0, 0, 0, 0}}},
        {"acc", "sequence 1 is not defined: the sequences must be exactly 0 .. S-1", {one, {BX_CONS_RATIO, 0, 0, 0, 0}, {BX_CONS_RATIO, 2, 0, 0, 0}}},
        {"acc", "sequence 1024 is not below BX_ACC_MAX_SEQS = 1024", {one, {BX_CONS_RATIO, 1024, 0, 0, 0}}},
        {"acc", "operand a = 7 refers to a later or missing fp var", {one, {BX_CONS_RATIO, 0, 7, 0, 0}}},
        {"acc", "operand b = 9 refers to a later or missing fp var", {one, {BX_CONS_RATIO, 0, 0, 9, 0}}},
        {"acc", "step 1: unknown op 13", {one, {13, 0, 0, 0, 0}}},
        {"acc", "step 1: unknown op 14", {one, {14, 0, 0, 0, 0}}},
        {"acc", "step 1: unknown op 15", {one, {15, 0, 0, 0, 0}}},
        {"acc", "step 1: unknown op 99", {one, {99, 0, 0, 0, 0}}},
        {"cons", "step 1: unknown op 16", {one, {BX_CONS_RATIO, 0, 0, 0, 0}}},
        {"wit", "step 1: unknown op 16", {one, {BX_CONS_RATIO, 0, 0, 0, 0}}},
    };
    for (const R& r : rs) {
        const char* msg;
        void* left = nullptr;
        if (!strcmp(r.who, "acc")) {
            bx_acc_program_desc d{r.steps.data(), r.steps.size(), nullptr, 0, 0};
            bx_acc_program* prog = nullptr;
            msg = bx_acc_program_create(&d, &prog);
            left = prog;
        } else if (!strcmp(r.who, "cons")) {
            bx_cons_program_desc d{};
            d.steps = r.steps.data(), d.n_steps = r.steps.size();
            bx_cons_program* prog = nullptr;
            msg = bx_cons_program_create(&d, &prog);
            left = prog;
        } else {
            bx_wit_program_desc d{};
            d.steps = r.steps.data(), d.n_steps = r.steps.size();
            bx_wit_program* prog = nullptr;
            msg = bx_wit_program_create(&d, &prog);
            left = prog;
        }
        if (!msg || left || !strstr(msg, r.want)) {
            printf("%s: wanted the refusal \"%s\", got: %s\n", r.who, r.want, msg ? msg : "(accepted)");
            return 1;
        }
    }
    // the most sequences there can be, all of them ratios
    {
        std::vector<bx_cons_step> steps{one};
        for (uint32_t s = 0; s < BX_ACC_MAX_SEQS; ++s) steps.push_back(bx_cons_step{BX_CONS_RATIO, s, 0, 0, 0});
        bx_acc_program_desc d{steps.data(), steps.size(), nullptr, 0, 0};
        bx_acc_program* prog = nullptr;
        if (const char* msg = bx_acc_program_create(&d, &prog)) return fail("1024 ratios", msg);
        bx_acc_program_info info;
        uint32_t R = 0;
        bx_acc_program_info_get(prog, &info);
        const char* e = bx_acc_program_ratios(prog, &R);
        const bool nulls_refused = bx_acc_program_ratios(nullptr, &R) && bx_acc_program_ratios(prog, nullptr);
        bx_acc_program_destroy(prog);
        if (e || R != BX_ACC_MAX_SEQS || info.sequences != BX_ACC_MAX_SEQS || info.sums != 0 || info.instructions != 1 + 2 * BX_ACC_MAX_SEQS) return fail("1024 ratios", "info is wrong");
        if (!nulls_refused) return fail("bx_acc_program_ratios", "took a null argument");
    }
    return 0;
}

int main() {
    if (refusals()) return 1;
    long compiled = 0, refused = 0, compiled_malformed = 0, ext_dens = 0, zero_dens = 0, n_ratios = 0;
    for (uint32_t seed = 0; seed < 3000; ++seed) {
        g_state = 0x4A710ull * (seed + 1);
        const bool bad = seed % 3 == 2;
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
        uint32_t S = 0, sums = 0, R = 0, got_R = ~0u;
        for (const bx_cons_step& s : c.steps) S += s.op == BX_CONS_SUM || s.op == BX_CONS_PROD || s.op == BX_CONS_RATIO, sums += s.op == BX_CONS_SUM, R += s.op == BX_CONS_RATIO;
        if (bx_acc_program_ratios(prog, &got_R) || got_R != R || info.steps != c.steps.size() || info.sequences != S || info.sums != sums ||
            info.instructions != c.steps.size() + R || info.taps != c.taps.size() || info.narrow > BX_CONS_MAX_NARROW || info.wide > BX_CONS_MAX_WIDE) {
            printf("seed %u: info is wrong (steps %u, sequences %u, sums %u, ratios %u, instructions %u)\n", seed, info.steps, info.sequences, info.sums, got_R, info.instructions);
            return 1;
        }
        n_ratios += R;
        bool fits = true;
        for (uint32_t k = 0; k < info.kept; ++k) {
            uint32_t g = 9, col = 9;
            if (bx_acc_program_kept(prog, k, &g, &col)) return fail("kept", "refused an index below info.kept");
            fits &= col < (g == 0 ? W_CODE : W_DATA);
        }
        const uint32_t wa = 4 * S + SPARE;
        for (uint32_t po2 : {1u, 3u, 6u})
            for (uint32_t kind = 0; kind < 4; ++kind) {
                if (po2 != 3 && kind && seed % 4) continue;  // every column pattern at po2 3; the rest for a quarter of the seeds
                const size_t n = (size_t)1 << po2;
                std::vector<uint32_t> code(W_CODE * n), data(W_DATA * n), gm(64 + 4);
                fill(code, kind);
                fill(data, kind);
                fill(gm, kind == 3 ? 0 : kind);
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
                            const Fp4& d4 = t.kind == SUM ? t.v : t.den;
                            Fp4 x = f4_zero();  // 1 / d with 0 -> 0; d * x = 1 is CHECKED here, whatever produced x
                            if (t.kind != PROD && !f4_is_zero(d4)) {
                                x = f4_inv(d4);
                                const Fp4 one = f4_mul(x, d4);
                                if (one.c[0] != MONT_ONE || one.c[1] || one.c[2] || one.c[3]) throw std::runtime_error("an inverse times its argument is not one");
                            }
                            if (t.kind == SUM) acc[s] = f4_add(r ? acc[s] : f4_zero(), f4_scale(x, t.m));
                            else if (t.kind == PROD) acc[s] = r ? f4_mul(acc[s], t.v) : t.v;
                            else {
                                const Fp4 q = f4_mul(t.v, x);
                                acc[s] = r ? f4_mul(acc[s], q) : q;
                                ext_dens += (d4.c[1] | d4.c[2] | d4.c[3]) != 0;
                                zero_dens += f4_is_zero(d4);
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
                    printf("seed %u po2 %u pattern %u: accum[%zu][%zu] is %u by the compiled stream, %u by the step list; %zu steps\n", seed, po2, kind, k / n, k % n, got[k],
                           want[k], c.steps.size());
                    return 1;
                }
            }
        bx_acc_program_destroy(prog);
    }
    printf("compiled %ld (of them malformed-but-valid %ld), refused %ld, ratios %ld, ext denominators %ld, zero denominators %ld\n", compiled, compiled_malformed, refused,
           n_ratios, ext_dens, zero_dens);
    if (compiled < 500 || refused < 300 || n_ratios < 1000 || ext_dens < 500 || zero_dens < 50) {
        printf("the case mix is too thin to mean anything\n");
        return 1;
    }
    printf("acc_ratio_check ok\n");
    return 0;
}
