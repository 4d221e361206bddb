// program_stream_pins.cpp — what the step-list compiler of csrc/program_compile.cpp (linked with csrc/cons_program_host.cpp, as
// every checker is) makes of seeded random descriptions, one line per description: the pin that a change to the compiler is
// checked against (tests/golden/progstream/pins.txt; README.md beside it gives the command).  Stand-alone, no HIP; tests/test_program_stream_pins_cpu.py builds it with -fsanitize=address,undefined.
//
// For each of the three kinds (constraint, witness, accumulate) a generator writes N_EACH descriptions: random step lists, tap lists,
// cells and count lists that keep the rules of include/bx_program.h, about half of them then broken on purpose by one or two
// mutations, each of which breaks one named rule.  A description that compiles prints a SHA-256 over the compiled form taken field
// by field, each field led by its name (never a memory image: padding and pointers play no part); one that is refused prints the
// full refusal.  The last line counts what the descriptions covered; the test asserts those counts.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "cons_program.hpp"
#include "fp.hpp"
#include "sha256_suite.hpp"

using namespace bx;

namespace {

constexpr int N_EACH = 400;
enum Kind { CONS = 0, WIT = 1, ACC = 2 };
const char* const kKind[3] = {"cons", "wit", "acc"};

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return n ? (uint32_t)(next() % n) : 0u; }
    bool chance(uint32_t percent) { return below(100) < percent; }
};

struct Count {
    uint32_t col, bins, rows;
    std::vector<uint32_t> sources;
};

struct Desc {
    std::vector<bx_cons_step> steps;
    std::vector<bx_cons_tap> taps;
    uint32_t n_globals = 0, ret = 0;
    std::vector<bx_wit_global_cell> cells;
    std::vector<Count> counts;
    bool null_steps = false, null_counts = false;
    // what the generator knows of it
    uint32_t n_fp = 0, n_mix = 0;
    int faults = 0;
};

struct Var {
    bool ext = false;
    uint32_t deg = 0;
    bool usable = true;  // false: the generator never names it again (a forwarded GET that nothing reads)
};

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t FREE_COLS = 10;  // witness programs: data columns below are free, derived ones start here

struct Gen {
    Rng& r;
    Desc& d;
    Kind kind;
    uint32_t window;
    std::vector<Var> fp;
    std::vector<uint32_t> free_taps;  // witness: the taps a GET may name before any SET

    uint32_t pick(bool want_base = false) {
        const uint32_t n = (uint32_t)fp.size();
        if (!n) return NONE;
        const uint32_t lo = n > window ? n - window : 0u;
        for (int k = 0; k < 8; ++k) {
            const uint32_t v = r.chance(5) ? r.below(n) : lo + r.below(n - lo);
            if (fp[v].usable && !(want_base && fp[v].ext)) return v;
        }
        for (uint32_t v = n; v-- > 0;)
            if (fp[v].usable && !(want_base && fp[v].ext)) return v;
        return NONE;
    }
    void push(const bx_cons_step& s, const Var& v) {
        d.steps.push_back(s);
        fp.push_back(v);
    }
    void constant() { push(bx_cons_step{BX_CONS_CONST, r.below(P), 0, 0, 0}, Var{}); }
    void value_step() {
        const uint32_t k = r.below(100);
        Var v;
        if (fp.size() < 2 || k < 10) return constant();
        if (k < 20 && kind != WIT) {
            v.ext = true;
            return push(bx_cons_step{BX_CONS_CONST_EXT, r.below(P), r.below(P), r.below(P), r.below(P)}, v);
        }
        if (k < 42) {
            const std::vector<uint32_t>* from = kind == WIT ? &free_taps : nullptr;
            const uint32_t n = from ? (uint32_t)from->size() : (uint32_t)d.taps.size();
            if (!n) return constant();
            const uint32_t t = r.below(n);
            v.deg = 1;
            return push(bx_cons_step{BX_CONS_GET, from ? (*from)[t] : t, 0, 0, 0}, v);
        }
        if (k < 50 && kind != WIT) {
            if (d.n_globals && r.chance(50)) return push(bx_cons_step{BX_CONS_GET_GLOBAL, 0, r.below(d.n_globals), 0, 0}, v);
            return push(bx_cons_step{BX_CONS_GET_GLOBAL, 1, r.below(4), 0, 0}, v);
        }
        const uint32_t a = pick(), b = pick();
        if (a == NONE || b == NONE) return constant();
        uint32_t op = BX_CONS_ADD + r.below(3);
        if (op == BX_CONS_MUL && kind == CONS && fp[a].deg + fp[b].deg > 3) op = BX_CONS_ADD + r.below(2);
        v.ext = fp[a].ext || fp[b].ext;
        v.deg = kind != CONS ? 0 : (op == BX_CONS_MUL ? fp[a].deg + fp[b].deg : std::max(fp[a].deg, fp[b].deg));
        push(bx_cons_step{op, a, b, 0, 0}, v);
    }
};

void gen_taps(Rng& r, Desc& d, uint32_t groups, uint32_t cols) {
    const uint32_t n = 1 + r.below(12);
    for (uint32_t t = 0; t < n; ++t) d.taps.push_back(bx_cons_tap{r.below(groups), r.below(cols), r.chance(50) ? 0u : r.below(4)});
}

uint32_t gen_size(Rng& r) { return r.chance(25) ? 100 + r.below(300) : 4 + r.below(60); }
uint32_t gen_window(Rng& r) { return r.chance(12) ? 40 + r.below(60) : 4 + r.below(10); }

void gen_cons(Rng& r, Desc& d) {
    gen_taps(r, d, 3, 20);
    d.n_globals = r.below(5);
    Gen g{r, d, CONS, gen_window(r), {}, {}};
    struct Mix {
        uint32_t deg;
    };
    std::vector<Mix> mix;
    const uint32_t n = gen_size(r);
    d.steps.push_back(bx_cons_step{BX_CONS_TRUE, 0, 0, 0, 0});
    mix.push_back(Mix{0});
    while (d.steps.size() < n) {
        const uint32_t k = r.below(100);
        const uint32_t x = r.chance(80) ? (uint32_t)mix.size() - 1 : (uint32_t)mix.size() - 1 - r.below(std::min<uint32_t>(3, (uint32_t)mix.size()));
        const uint32_t y = g.pick();
        if (k < 3) {
            d.steps.push_back(bx_cons_step{BX_CONS_TRUE, 0, 0, 0, 0});
            mix.push_back(Mix{0});
        } else if (k < 9 && y != NONE) {
            const uint32_t c = (uint32_t)mix.size() - 1 - r.below(std::min<uint32_t>(3, (uint32_t)mix.size()));
            if (g.fp[y].deg + mix[c].deg > BX_CONS_MAX_DEGREE) continue;
            d.steps.push_back(bx_cons_step{BX_CONS_AND_COND, x, y, c, 0});
            mix.push_back(Mix{std::max(mix[x].deg, g.fp[y].deg + mix[c].deg)});
        } else if (k < 22 && y != NONE) {
            d.steps.push_back(bx_cons_step{BX_CONS_AND_EQZ, x, y, 0, 0});
            mix.push_back(Mix{std::max(mix[x].deg, g.fp[y].deg)});
        } else {
            g.value_step();
        }
    }
    d.n_fp = (uint32_t)g.fp.size();
    d.n_mix = (uint32_t)mix.size();
    d.ret = d.n_mix - 1;
}

void gen_wit(Rng& r, Desc& d) {
    Gen g{r, d, WIT, gen_window(r), {}, {}};
    gen_taps(r, d, 2, FREE_COLS);
    for (uint32_t t = 0; t < d.taps.size(); ++t) g.free_taps.push_back(t);
    const uint32_t n_derived = r.below(7);
    std::vector<uint32_t> derived_tap;  // per planned derived column FREE_COLS + k: its back-0 tap, or NONE
    for (uint32_t k = 0; k < n_derived; ++k) {
        derived_tap.push_back(r.chance(75) ? (uint32_t)d.taps.size() : NONE);
        if (derived_tap.back() != NONE) d.taps.push_back(bx_cons_tap{1, FREE_COLS + k, 0});
    }
    uint32_t n_set = 0;
    const uint32_t n = gen_size(r);
    while (d.steps.size() < n) {
        const uint32_t k = r.below(100);
        if (k < 12 && n_set < n_derived && g.pick() != NONE) {
            d.steps.push_back(bx_cons_step{BX_CONS_SET, FREE_COLS + n_set, g.pick(), 0, 0});
            ++n_set;
        } else if (k < 24 && n_set) {
            const uint32_t t = derived_tap[r.below(n_set)];
            if (t == NONE) continue;
            Var v;
            v.usable = !r.chance(30);
            g.push(bx_cons_step{BX_CONS_GET, t, 0, 0, 0}, v);
        } else {
            g.value_step();
        }
    }
    d.n_fp = (uint32_t)g.fp.size();
    const uint32_t n_cells = r.chance(50) ? r.below(4) : 0u;
    for (uint32_t k = 0; k < n_cells; ++k) d.cells.push_back(bx_wit_global_cell{k * 7 + r.below(7), r.below(20), r.below(64)});
    const uint32_t n_counts = r.chance(50) ? r.below(4) : 0u;
    for (uint32_t k = 0; k < n_counts; ++k) {
        Count c{30 + 3 * k + r.below(3), 1 + r.below(16), 0, {}};
        if (r.chance(50)) c.rows = c.bins + r.below(100);
        const uint32_t ns = 1 + r.below(4);
        for (uint32_t q = 0; q < ns; ++q) c.sources.push_back(q * 5 + r.below(5));  // free or SET columns, each once
        d.counts.push_back(c);
    }
}

void gen_acc(Rng& r, Desc& d) {
    gen_taps(r, d, 2, 20);
    d.n_globals = r.below(5);
    Gen g{r, d, ACC, gen_window(r), {}, {}};
    const uint32_t S = 1 + r.below(10), sums = r.below(S + 1);
    std::vector<uint32_t> ids(S);
    for (uint32_t s = 0; s < S; ++s) ids[s] = s;
    for (uint32_t s = S; s > 1; --s) std::swap(ids[s - 1], ids[r.below(s)]);
    const uint32_t n = gen_size(r);
    uint32_t next = 0;
    const auto term = [&] {
        const uint32_t s = ids[next++];
        if (s < sums) {
            if (g.pick(true) == NONE) g.constant();
            d.steps.push_back(bx_cons_step{BX_CONS_SUM, s, g.pick(true), g.pick(), 0});
        } else {
            d.steps.push_back(bx_cons_step{BX_CONS_PROD, s, g.pick(), 0, 0});
        }
    };
    g.constant();
    while (d.steps.size() < n) {
        if (next < S && g.fp.size() > 3 && r.below(n) < 2 * S) term();
        else g.value_step();
    }
    while (next < S) term();
    d.n_fp = (uint32_t)g.fp.size();
}

// ---- mutations: each breaks one rule of the text; false = this description has nothing the mutation applies to ----
uint32_t find_step(Rng& r, const Desc& d, uint32_t op_lo, uint32_t op_hi) {
    std::vector<uint32_t> at;
    for (uint32_t i = 0; i < d.steps.size(); ++i)
        if (d.steps[i].op >= op_lo && d.steps[i].op <= op_hi) at.push_back(i);
    return at.empty() ? NONE : at[r.below((uint32_t)at.size())];
}

bool mutate_count(Rng& r, Desc& d) {
    if (d.counts.empty()) d.counts.push_back(Count{40, 4, 0, {0, 1}});
    Count& c = d.counts[r.below((uint32_t)d.counts.size())];
    switch (r.below(15)) {
    case 0: c.bins = 0; return true;
    case 1: c.bins = (1u << 24) + 1 + r.below(9); return true;
    case 2: c.rows = (1u << 24) + 1 + r.below(9); return true;
    case 3: c.rows = 1 + r.below(50), c.bins = c.rows + 1 + r.below(9); return true;
    case 4: c.sources.clear(); return true;
    case 5: {
        const uint32_t n = BX_WIT_MAX_COUNT_SOURCES + 1 + r.below(3);
        c.sources.clear();
        for (uint32_t q = 0; q < n; ++q) c.sources.push_back(100 + q);
        return true;
    }
    case 6:
        if (c.sources.empty()) c.sources.push_back(3);
        c.sources.push_back(c.sources[r.below((uint32_t)c.sources.size())]);
        return true;
    case 7: c.sources.push_back(65536 + r.below(9)); return true;
    case 8: c.col = 65536 + r.below(9); return true;
    case 9: {
        const uint32_t i = find_step(r, d, BX_CONS_SET, BX_CONS_SET);
        if (i == NONE) return false;
        c.col = d.steps[i].a;
        return true;
    }
    case 10:
        d.taps.push_back(bx_cons_tap{1, c.col, r.below(3)});
        d.steps.push_back(bx_cons_step{BX_CONS_GET, (uint32_t)d.taps.size() - 1, 0, 0, 0});
        return true;
    case 11: d.counts[r.below((uint32_t)d.counts.size())].sources.push_back(c.col); return true;
    case 12: {
        const Count copy = c;
        d.counts.push_back(copy);
        d.counts.back().sources.assign(1, 9);
        return true;
    }
    case 13:
        while (d.counts.size() < 17) d.counts.push_back(Count{200 + (uint32_t)d.counts.size(), 2, 0, {1}});
        return true;
    default: d.null_counts = true; return true;
    }
}

bool mutate(Rng& r, Desc& d, Kind kind) {
    const uint32_t own = kind == CONS ? 4 : (kind == WIT ? 14 : 6);
    const uint32_t m = r.below(12 + own);
    if ((m == 7 || m >= 9) && m < 12 && !r.chance(25)) return false;  // the rules that are judged first hide every other one: fewer of them
    uint32_t i;
    switch (m) {
    case 0:
        if (d.taps.empty()) return false;
        d.taps[r.below((uint32_t)d.taps.size())].group = kind == CONS ? 3 + r.below(3) : 2 + r.below(2);
        return true;
    case 1:
        if (d.taps.empty()) return false;
        d.taps[r.below((uint32_t)d.taps.size())].col = 65536 + r.below(9);
        return true;
    case 2:
        if (d.taps.empty()) return false;
        d.taps[r.below((uint32_t)d.taps.size())].back = 65536 + r.below(9);
        return true;
    case 3:
        i = find_step(r, d, BX_CONS_CONST, kind == WIT ? BX_CONS_CONST : BX_CONS_CONST_EXT);
        if (i == NONE) return false;
        (r.chance(50) || d.steps[i].op == BX_CONS_CONST ? d.steps[i].a : d.steps[i].c) = P + r.below(5);
        return true;
    case 4:
        i = find_step(r, d, BX_CONS_ADD, BX_CONS_MUL);
        if (i == NONE) return false;
        (r.chance(50) ? d.steps[i].a : d.steps[i].b) = r.chance(50) ? d.n_fp + r.below(3) : 1000000u;
        return true;
    case 5:
        i = find_step(r, d, BX_CONS_GET, BX_CONS_GET);
        if (i == NONE) return false;
        d.steps[i].a = (uint32_t)d.taps.size() + r.below(3);
        return true;
    case 6: {
        static const uint32_t cons_ops[] = {10, 11, 12, 13, 99}, wit_ops[] = {1, 3, 7, 8, 9, 11, 12, 13, 99}, acc_ops[] = {7, 8, 9, 10, 13, 99};
        if (d.steps.empty()) return false;
        bx_cons_step& s = d.steps[r.below((uint32_t)d.steps.size())];
        s.op = kind == CONS ? cons_ops[r.below(5)] : (kind == WIT ? wit_ops[r.below(9)] : acc_ops[r.below(6)]);
        return true;
    }
    case 7:
        if (kind == WIT) {
            while (d.cells.size() <= BX_MAX_GLOBALS) d.cells.push_back(bx_wit_global_cell{(uint32_t)d.cells.size(), 1, 1});
        } else {
            d.n_globals = BX_MAX_GLOBALS + 1 + r.below(9);
        }
        return true;
    case 8:
        if (kind == WIT) return false;
        i = find_step(r, d, BX_CONS_CONST, BX_CONS_CONST);
        if (i == NONE) return false;
        d.steps[i].op = BX_CONS_GET_GLOBAL;
        switch (r.below(3)) {
        case 0: d.steps[i].a = 2 + r.below(3); break;
        case 1: d.steps[i].a = 0, d.steps[i].b = d.n_globals + r.below(3); break;
        default: d.steps[i].a = 1, d.steps[i].b = 4 + r.below(3); break;
        }
        return true;
    case 9:
        if (d.steps.empty()) return false;
        d.null_steps = true;
        return true;
    case 10:
        d.steps.resize(BX_CONS_MAX_STEPS + 1 + r.below(3), bx_cons_step{BX_CONS_CONST, 0, 0, 0, 0});
        return true;
    case 11:
        d.taps.resize(BX_CONS_MAX_TAPS + 1 + r.below(3), bx_cons_tap{0, 0, 0});
        return true;
    default: break;
    }
    const uint32_t k = m - 12;
    if (kind == CONS) {
        switch (k) {
        case 0: d.ret = d.n_mix + r.below(3); return true;
        case 1:
            i = find_step(r, d, BX_CONS_AND_EQZ, BX_CONS_AND_COND);
            if (i == NONE) return false;
            (r.chance(50) ? d.steps[i].a : d.steps[i].b) = 500000u + r.below(3);
            return true;
        case 2: {  // x^6 is above the degree bound
            if (d.taps.empty()) return false;
            const uint32_t v = d.n_fp;
            d.steps.push_back(bx_cons_step{BX_CONS_GET, r.below((uint32_t)d.taps.size()), 0, 0, 0});
            d.steps.push_back(bx_cons_step{BX_CONS_MUL, v, v, 0, 0});
            d.steps.push_back(bx_cons_step{BX_CONS_MUL, v + 1, v + 1, 0, 0});
            d.steps.push_back(bx_cons_step{BX_CONS_MUL, v + 2, v + 1, 0, 0});
            d.n_fp += 4;
            return true;
        }
        default: {  // nine distinct backs on one column
            const uint32_t g = r.below(3), col = 21 + r.below(5);
            for (uint32_t b = 1; b <= BX_MAX_TAPS; ++b) d.taps.push_back(bx_cons_tap{g, col, b});
            return true;
        }
        }
    }
    if (kind == WIT) {
        switch (k) {
        case 0:
            i = find_step(r, d, BX_CONS_SET, BX_CONS_SET);
            if (i == NONE) return false;
            d.steps.push_back(d.steps[i]);
            return true;
        case 1:
            i = find_step(r, d, BX_CONS_SET, BX_CONS_SET);
            if (i == NONE) return false;
            d.taps.push_back(bx_cons_tap{1, d.steps[i].a, 1 + r.below(3)});
            d.steps.push_back(bx_cons_step{BX_CONS_GET, (uint32_t)d.taps.size() - 1, 0, 0, 0});
            return true;
        case 2: {  // a GET of a derived column before its SET: a CONST in front of the SET becomes that GET
            i = find_step(r, d, BX_CONS_SET, BX_CONS_SET);
            if (i == NONE) return false;
            uint32_t c = NONE;
            for (uint32_t j = 0; j < i && c == NONE; ++j)
                if (d.steps[j].op == BX_CONS_CONST) c = j;
            if (c == NONE) return false;
            d.taps.push_back(bx_cons_tap{1, d.steps[i].a, 0});
            d.steps[c] = bx_cons_step{BX_CONS_GET, (uint32_t)d.taps.size() - 1, 0, 0, 0};
            return true;
        }
        case 3:
            if (d.cells.empty()) d.cells.push_back(bx_wit_global_cell{r.below(20), 2, 2});
            d.cells.push_back(d.cells[r.below((uint32_t)d.cells.size())]);
            return true;
        case 4: d.cells.push_back(bx_wit_global_cell{BX_MAX_GLOBALS + r.below(3), 1, 1}); return true;
        case 5: d.cells.push_back(bx_wit_global_cell{60 + r.below(4), 65536 + r.below(3), 1}); return true;
        default: return mutate_count(r, d);
        }
    }
    std::vector<uint32_t> terms, sum_at, prod_at;
    for (uint32_t j = 0; j < d.steps.size(); ++j) {
        if (d.steps[j].op == BX_CONS_SUM) sum_at.push_back(j), terms.push_back(j);
        if (d.steps[j].op == BX_CONS_PROD) prod_at.push_back(j), terms.push_back(j);
    }
    if (terms.empty()) return false;
    switch (k) {
    case 0: d.steps.push_back(d.steps[terms[r.below((uint32_t)terms.size())]]); return true;
    case 1: d.steps[terms[r.below((uint32_t)terms.size())]].a = (uint32_t)terms.size() + 1 + r.below(5); return true;
    case 2:
        if (sum_at.empty() || prod_at.empty()) return false;
        std::swap(d.steps[sum_at[r.below((uint32_t)sum_at.size())]].a, d.steps[prod_at[r.below((uint32_t)prod_at.size())]].a);
        return true;
    case 3: {  // an ext-typed m: the SUM moves behind a new ext constant and names it
        if (sum_at.empty()) return false;
        const uint32_t at = sum_at[r.below((uint32_t)sum_at.size())];
        bx_cons_step s = d.steps[at];
        d.steps.erase(d.steps.begin() + at);
        d.steps.push_back(bx_cons_step{BX_CONS_CONST_EXT, 1, 2, 3, 4});
        s.b = d.n_fp++;
        d.steps.push_back(s);
        return true;
    }
    case 4: d.steps[terms[r.below((uint32_t)terms.size())]].a = BX_ACC_MAX_SEQS + r.below(3); return true;
    default:
        for (size_t j = terms.size(); j-- > 0;) d.steps.erase(d.steps.begin() + terms[j]);
        return true;
    }
}

// ---- the compiled form, field by field ----
struct Hash {
    Sha256 h;
    void word(uint32_t w) {
        const uint8_t b[4] = {(uint8_t)w, (uint8_t)(w >> 8), (uint8_t)(w >> 16), (uint8_t)(w >> 24)};
        h.update(b, 4);
    }
    void name(const char* n) { h.update((const uint8_t*)n, strlen(n) + 1); }
    void field(const char* n, uint32_t v) { name(n), word(v); }
    void list(const char* n, const std::vector<uint32_t>& v) {
        field(n, (uint32_t)v.size());
        for (uint32_t w : v) word(w);
    }
    void taps(const char* n, const std::vector<bx_cons_tap>& v) {
        field(n, (uint32_t)v.size());
        for (const bx_cons_tap& t : v) word(t.group), word(t.col), word(t.back);
    }
    std::string hex() {
        uint8_t out[32];
        h.finish(out);
        char s[65];
        for (int k = 0; k < 32; ++k) snprintf(s + 2 * k, 3, "%02x", out[k]);
        return s;
    }
};

std::string hash_of(const bx_cons_program* p) {
    Hash h;
    const bx_cons_program_info& in = p->info;
    h.field("info.steps", in.steps), h.field("info.constraints", in.constraints), h.field("info.degree", in.degree), h.field("info.narrow", in.narrow);
    h.field("info.wide", in.wide), h.field("info.instructions", in.instructions), h.field("info.taps", in.taps), h.field("info.n_globals", in.n_globals);
    h.list("code", p->code), h.list("consts", p->consts), h.taps("taps", p->taps);
    h.field("n_pows", p->n_pows), h.field("ret_slot", p->ret_slot);
    h.name("max_col");
    for (uint32_t m : p->max_col) h.word(m);
    return h.hex();
}
std::string hash_of(const bx_wit_program* p) {
    Hash h;
    const bx_wit_program_info& in = p->info;
    h.field("info.steps", in.steps), h.field("info.sets", in.sets), h.field("info.narrow", in.narrow), h.field("info.instructions", in.instructions);
    h.field("info.taps", in.taps), h.field("info.cells", in.cells);
    h.list("code", p->code), h.list("consts", p->consts), h.taps("taps", p->taps), h.list("sets", p->sets);
    h.field("cells", (uint32_t)p->cells.size());
    for (const bx_wit_global_cell& g : p->cells) h.word(g.global), h.word(g.col), h.word(g.row);
    h.name("max_col");
    for (uint32_t m : p->max_col) h.word(m);
    h.field("max_set", p->max_set);
    h.field("counts", (uint32_t)p->counts.size());
    for (const WitCount& c : p->counts) h.field("col", c.col), h.field("bins", c.bins), h.field("rows", c.rows), h.list("sources", c.sources);
    return h.hex();
}
std::string hash_of(const bx_acc_program* p) {
    Hash h;
    const bx_acc_program_info& in = p->info;
    h.field("info.steps", in.steps), h.field("info.sequences", in.sequences), h.field("info.sums", in.sums), h.field("info.instructions", in.instructions);
    h.field("info.narrow", in.narrow), h.field("info.wide", in.wide), h.field("info.taps", in.taps), h.field("info.kept", in.kept), h.field("info.n_globals", in.n_globals);
    h.list("code", p->code), h.list("consts", p->consts), h.taps("taps", p->taps), h.list("tap_kept", p->tap_kept), h.taps("kept", p->kept);
    return h.hex();
}

bool has_ops(const std::vector<uint32_t>& code, std::initializer_list<uint32_t> ops) {
    for (uint32_t op : ops) {
        bool found = false;
        for (size_t pc = 0; pc < code.size() && !found; pc += 2) found = (code[pc] & 0xFFu) == op;
        if (!found) return false;
    }
    return true;
}
const std::initializer_list<uint32_t> kMixedOps = {CP_ADD_EB, CP_SUB_EB, CP_SUB_BE, CP_MUL_EB};

struct Tally {
    int ok = 0, refused = 0, reuse = 0, mixed = 0, forwarded = 0, dead_forward = 0, all_terms = 0, two_faults_refused = 0;
};

// an accepted witness description: has it a forwarded GET, and one that no later step reads
void forwards(const Desc& d, bool* any, bool* dead) {
    std::vector<uint32_t> var_step;  // fp var -> its step
    for (uint32_t i = 0; i < d.steps.size(); ++i)
        if (d.steps[i].op != BX_CONS_SET) var_step.push_back(i);
    for (uint32_t v = 0; v < var_step.size(); ++v) {
        const bx_cons_step& s = d.steps[var_step[v]];
        if (s.op != BX_CONS_GET || d.taps[s.a].group != 1) continue;
        bool derived = false;
        for (uint32_t j = 0; j < var_step[v]; ++j) derived |= d.steps[j].op == BX_CONS_SET && d.steps[j].a == d.taps[s.a].col;
        if (!derived) continue;
        *any = true;
        bool read = false;
        for (size_t j = var_step[v] + 1; j < d.steps.size(); ++j) {
            const bx_cons_step& u = d.steps[j];
            read |= (u.op >= BX_CONS_ADD && u.op <= BX_CONS_MUL && (u.a == v || u.b == v)) || (u.op == BX_CONS_SET && u.b == v);
        }
        if (!read) *dead = true;
    }
}

}  // namespace

int main() {
    Tally tally[3];
    for (int kind = 0; kind < 3; ++kind) {
        for (int n = 0; n < N_EACH; ++n) {
            Rng r{0x5EEDull * 1000003ull + (uint64_t)kind * 100000ull + (uint64_t)n};
            Desc d;
            if (kind == CONS) gen_cons(r, d);
            else if (kind == WIT) gen_wit(r, d);
            else gen_acc(r, d);
            const uint32_t want = r.chance(55) ? 0u : (r.chance(60) ? 1u : 2u);
            for (int tries = 0; d.faults < (int)want && tries < 50; ++tries) d.faults += mutate(r, d, (Kind)kind) ? 1 : 0;

            const bx_cons_step* steps = d.null_steps ? nullptr : d.steps.data();
            Tally& t = tally[kind];
            std::string line;
            const char* e;
            if (kind == CONS) {
                const bx_cons_program_desc desc{steps, d.steps.size(), d.taps.data(), d.taps.size(), d.n_globals, d.ret};
                bx_cons_program* p = nullptr;
                if (!(e = bx_cons_program_create(&desc, &p))) {
                    line = hash_of(p);
                    t.reuse += p->info.instructions > p->info.narrow + p->info.wide;
                    t.mixed += has_ops(p->code, kMixedOps) && has_ops(p->code, {CP_EQZ_B, CP_EQZ_E, CP_COND_B, CP_COND_E});
                    bx_cons_program_destroy(p);
                }
            } else if (kind == WIT) {
                std::vector<bx_wit_count> counts;
                for (const Count& c : d.counts) counts.push_back(bx_wit_count{c.col, c.bins, c.rows, (uint32_t)c.sources.size(), c.sources.data()});
                const bx_wit_program_desc desc{steps, d.steps.size(), d.taps.data(), d.taps.size(), d.cells.data(), d.cells.size()};
                bx_wit_program* p = nullptr;
                if (!(e = bx_wit_program_create_counted(&desc, d.null_counts ? nullptr : counts.data(), counts.size(), &p))) {
                    line = hash_of(p);
                    t.reuse += p->info.instructions > p->info.narrow;
                    bool any = false, dead = false;
                    forwards(d, &any, &dead);
                    t.forwarded += any, t.dead_forward += dead;
                    bx_wit_program_destroy(p);
                }
            } else {
                const bx_acc_program_desc desc{steps, d.steps.size(), d.taps.data(), d.taps.size(), d.n_globals};
                bx_acc_program* p = nullptr;
                if (!(e = bx_acc_program_create(&desc, &p))) {
                    line = hash_of(p);
                    t.reuse += p->info.instructions > p->info.narrow + p->info.wide;
                    t.mixed += has_ops(p->code, kMixedOps);
                    t.all_terms += has_ops(p->code, {CP_TSUM_B, CP_TSUM_E, CP_TPROD_B, CP_TPROD_E});
                    bx_acc_program_destroy(p);
                }
            }
            if (e) ++t.refused, t.two_faults_refused += d.faults >= 2;
            else ++t.ok;
            printf("%s %d %s %s\n", kKind[kind], n, e ? "refused" : "ok", e ? e : line.c_str());
        }
    }
    printf("summary cons ok=%d refused=%d reuse=%d mixed=%d two_faults_refused=%d | wit ok=%d refused=%d reuse=%d forwarded=%d dead_forward=%d two_faults_refused=%d | "
           "acc ok=%d refused=%d reuse=%d mixed=%d all_terms=%d two_faults_refused=%d\n",
           tally[0].ok, tally[0].refused, tally[0].reuse, tally[0].mixed, tally[0].two_faults_refused, tally[1].ok, tally[1].refused, tally[1].reuse, tally[1].forwarded,
           tally[1].dead_forward, tally[1].two_faults_refused, tally[2].ok, tally[2].refused, tally[2].reuse, tally[2].mixed, tally[2].all_terms,
           tally[2].two_faults_refused);
    return 0;
}
