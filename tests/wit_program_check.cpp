// wit_program_check.cpp — stand-alone checker of the witness-program compiler and host executor (csrc/program_compile.cpp, csrc/cons_program_host.cpp), built with
// -fsanitize=address,undefined by tests/test_wit_program_cpu.py and run as a process of its own.
//
// Seeded descriptors, well-formed and malformed, go through bx_wit_program_create.  Every one is either refused (with a message) or
// compiled; every compiled stream, run by bx_wit_program_run_host at po2 1, 3 and 6 over random and extreme free columns, must agree
// with a DIRECT evaluation of the step list — every var a cell of its own, no slot file, no forwarding (a GET of a derived column reads
// the word its SET stored), written below and sharing only the field arithmetic of fp.hpp with the library.  That is the slot
// allocator's invariant: no live value is overwritten, and a forwarded value is still there when it is named.  The direct evaluation
// also states the three derived-column rules itself and throws when create let a program through that breaks one.
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

constexpr uint32_t W_CODE = 3, W_DATA = 8;

struct Case {
    std::vector<bx_cons_step> steps;
    std::vector<bx_cons_tap> taps;
    std::vector<bx_wit_global_cell> cells;
};

// the header's table, literally, for one row r of column-major matrices (`data` in place); .at() throws if create let an operand
// through that names nothing
static void direct_row(const Case& c, const std::map<uint32_t, size_t>& set_at, uint32_t po2, uint32_t r, const std::vector<uint32_t>& code,
                       std::vector<uint32_t>& data) {
    const uint32_t n = 1u << po2;
    std::vector<uint32_t> fp;
    for (size_t i = 0; i < c.steps.size(); ++i) {
        const bx_cons_step& s = c.steps[i];
        switch (s.op) {
        case BX_CONS_CONST: fp.push_back(fp_encode(s.a)); break;
        case BX_CONS_GET: {
            const bx_cons_tap& t = c.taps.at(s.a);
            if (t.group > 1) throw std::runtime_error("create accepted a tap of a group that does not exist at witgen time");
            if (t.group == 1 && set_at.count(t.col)) {
                if (t.back) throw std::runtime_error("create accepted a GET of a derived column on another row");
                if (set_at.at(t.col) > i) throw std::runtime_error("create accepted a GET of a derived column before its SET");
            }
            const std::vector<uint32_t>& g = t.group == 0 ? code : data;
            fp.push_back(g.at((size_t)t.col * n + ((r - t.back) & (n - 1u))));
            break;
        }
        case BX_CONS_ADD: fp.push_back(fp_add(fp.at(s.a), fp.at(s.b))); break;
        case BX_CONS_SUB: fp.push_back(fp_sub(fp.at(s.a), fp.at(s.b))); break;
        case BX_CONS_MUL: fp.push_back(fp_mul(fp.at(s.a), fp.at(s.b))); break;
        case BX_CONS_SET:
            if (set_at.at(s.a) != i) throw std::runtime_error("create accepted a second SET of a column");
            data.at((size_t)s.a * n + r) = fp.at(s.b);
            break;
        default: throw std::runtime_error("create accepted an op that does not belong in a witness program");
        }
    }
}

// well-formed by construction except for live-value pressure, which create may refuse
static Case well_formed(uint32_t n_steps, uint32_t far_share) {
    Case c;
    std::vector<uint32_t> derived, free_cols, done;
    for (uint32_t col = 0; col < W_DATA; ++col) (col && below(2) ? derived : free_cols).push_back(col);  // column 0 is always free
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
            else c.steps.push_back(bx_cons_step{BX_CONS_GET, tap(1, free_cols[below((uint32_t)free_cols.size())], below(5)), 0, 0, 0});
        } else {
            const uint32_t r = below(3);
            c.steps.push_back(bx_cons_step{r == 0 ? BX_CONS_ADD : (r == 1 ? BX_CONS_SUB : BX_CONS_MUL), pick(), pick(), 0, 0});
        }
        ++n_fp;
    }
    for (uint32_t g = 0, n = below(3); g < n; ++g) c.cells.push_back(bx_wit_global_cell{g, below(W_DATA), below(2)});
    return c;
}
// a well-formed case with some fields overwritten by anything
static Case malformed() {
    Case c = well_formed(5 + below(60), 30);
    const uint32_t hits = 1 + below(3);
    for (uint32_t h = 0; h < hits; ++h) {
        bx_cons_step& s = c.steps[below((uint32_t)c.steps.size())];
        switch (below(8)) {
        case 0: s.op = below(14); break;
        case 1: s.a = (uint32_t)rnd() >> below(32); break;
        case 2: s.b = (uint32_t)rnd() >> below(32); break;
        case 3: c.taps[below((uint32_t)c.taps.size())] = bx_cons_tap{below(4), below(W_DATA), below(3)}; break;
        case 4: c.taps[below((uint32_t)c.taps.size())] = bx_cons_tap{below(5), (uint32_t)rnd() >> below(32), (uint32_t)rnd() >> below(32)}; break;
        case 5: c.cells.push_back(bx_wit_global_cell{(uint32_t)rnd() >> below(32), below(W_DATA), 0}); break;
        case 6: s = bx_cons_step{BX_CONS_SET, below(W_DATA), below(40), 0, 0}; break;
        default: s = bx_cons_step{below(12), below(40), below(40), below(40), (uint32_t)rnd()}; break;
        }
    }
    return c;
}

// free and code columns: random, all 0, all P - 1, alternating 0 / P - 1
static void fill(std::vector<uint32_t>& v, uint32_t kind) {
    for (size_t i = 0; i < v.size(); ++i) v[i] = kind == 0 ? below(P) : (kind == 1 ? 0u : (kind == 2 ? P - 1 : (i & 1 ? P - 1 : 0u)));
}

int main() {
    long compiled = 0, refused = 0, compiled_malformed = 0, forwarded = 0;
    uint32_t peak_narrow = 0;
    for (uint32_t seed = 0; seed < 3000; ++seed) {
        g_state = 0x317E55ull * (seed + 1);
        const bool bad = seed % 3 == 2;
        // short and long programs; mostly near operands (few live values: these compile), sometimes far ones (pressure: refusals)
        const Case c = bad ? malformed() : well_formed(seed % 7 == 0 ? 400 + below(600) : 3 + below(80), seed % 5 == 0 ? 25 : 2);
        bx_wit_program_desc d{c.steps.data(), c.steps.size(), c.taps.data(), c.taps.size(), c.cells.data(), c.cells.size()};
        bx_wit_program* prog = nullptr;
        const char* msg = bx_wit_program_create(&d, &prog);
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
        bx_wit_program_info info;
        bx_wit_program_info_get(prog, &info);
        std::map<uint32_t, size_t> set_at;
        uint32_t n_fwd = 0, n_fp_steps = 0;
        for (size_t i = 0; i < c.steps.size(); ++i)
            if (c.steps[i].op == BX_CONS_SET) set_at.emplace(c.steps[i].a, i);
        for (const bx_cons_step& s : c.steps) {
            n_fp_steps += s.op != BX_CONS_SET;
            n_fwd += s.op == BX_CONS_GET && s.a < c.taps.size() && c.taps[s.a].group == 1 && set_at.count(c.taps[s.a].col);
        }
        // one instruction per step, none for a forwarded GET
        if (info.narrow > BX_CONS_MAX_NARROW || info.steps != c.steps.size() || info.sets != set_at.size() || info.instructions != c.steps.size() - n_fwd ||
            info.cells != c.cells.size()) {
            printf("seed %u: info is wrong (narrow %u, steps %u, sets %u, instructions %u for %zu steps of which %u forwarded)\n", seed, info.narrow, info.steps,
                   info.sets, info.instructions, c.steps.size(), n_fwd);
            return 1;
        }
        for (uint32_t col = 0; col < W_DATA + 2; ++col)
            if (bx_wit_program_derives(prog, col) != (int)set_at.count(col)) {
                printf("seed %u: derives(%u) is wrong\n", seed, col);
                return 1;
            }
        forwarded += n_fwd;
        peak_narrow = info.narrow > peak_narrow ? info.narrow : peak_narrow;
        // a compiled malformed case may name columns beyond the widths used here: run_host must then refuse, by message
        bool fits = true;
        for (const bx_cons_tap& t : c.taps) fits &= t.col < (t.group == 0 ? W_CODE : W_DATA);
        for (const auto& kv : set_at) fits &= kv.first < W_DATA;
        for (uint32_t po2 : {1u, 3u, 6u})
            for (uint32_t kind = 0; kind < 4; ++kind) {
                if (po2 != 3 && kind && seed % 4) continue;  // every pattern at po2 3, and at the other two for a quarter of the seeds
                const size_t n = (size_t)1 << po2;
                std::vector<uint32_t> code(W_CODE * n), data(W_DATA * n);
                fill(code, kind);
                fill(data, kind);
                for (const auto& kv : set_at)
                    if (kv.first < W_DATA)
                        for (size_t r = 0; r < n; ++r) data[kv.first * n + r] = P - 1;  // derived columns: poisoned
                std::vector<uint32_t> got = data, want = data;
                const char* e = bx_wit_program_run_host(prog, po2, code.data(), W_CODE, got.data(), W_DATA);
                if (!fits) {
                    if (!e || !*e || got != data) {
                        printf("seed %u: run_host took a program that names a column beyond the widths, or wrote before it refused\n", seed);
                        return 1;
                    }
                    continue;
                }
                if (e) {
                    printf("seed %u: run_host: %s\n", seed, e);
                    return 1;
                }
                try {
                    for (uint32_t r = 0; r < n; ++r) direct_row(c, set_at, po2, (uint32_t)(n - 1 - r), code, want);  // rows in another order than the library's
                } catch (const std::exception& ex) {
                    printf("seed %u: create accepted a descriptor the definition cannot evaluate: %s\n", seed, ex.what());
                    return 1;
                }
                if (got != want) {
                    size_t k = 0;
                    while (got[k] == want[k]) ++k;
                    printf("seed %u po2 %u pattern %u: data[%zu][%zu] is %u by the compiled stream, %u by the step list; %zu steps, narrow %u\n", seed, po2, kind, k / n,
                           k % n, got[k], want[k], c.steps.size(), info.narrow);
                    return 1;
                }
            }
        bx_wit_program_destroy(prog);
    }
    printf("compiled %ld (of them malformed-but-valid %ld), refused %ld, forwarded GETs %ld, peak narrow %u\n", compiled, compiled_malformed, refused, forwarded,
           peak_narrow);
    if (compiled < 500 || refused < 300 || forwarded < 500 || peak_narrow < 8) {
        printf("the case mix is too thin to mean anything\n");
        return 1;
    }
    printf("wit_program_check ok\n");
    return 0;
}
