// seal_layout_check.cpp — the seal's layout (csrc/seal_layout.hpp) without a GPU; stand-alone, built with -fsanitize=address,undefined
// by tests/test_seal_layout_check_cpu.py.
//
//   seal_layout_check <cases.txt>
//
// 1. Against the C oracle, which shares no code with the layout.  Every line of cases.txt is a shape of the synthetic circuit, the
//    length of the seal oracle/ proved for it and that seal's first six words: the layout's seal_words must be that length, the
//    header the one the layout was built from, and queries_at + BX_QUERIES * per_query the whole seal.
// 2. Invariants, for every po2 in 9 .. 24 and group widths from {1, 2, 16, 256, 65535}, under the synthetic circuit's tap sets and
//    (where it takes the shape) the lookup circuit's: the FRI rounds end at or below the final degree, every tree's top layer follows
//    the rule, the tap counts add up, every column's combo holds exactly the column's tap set, and the lengths are the sums restated
//    here.  UBSan sees the products of the largest shapes.  Every po2 meets every combination of the four smaller widths and all
//    three groups at 65535; the mixed combinations with 65535 (196 605 columns walked twice under the sanitizers, 61 times per po2)
//    are met at po2 9 and 24 only: the size enters the per-column work through the bound on a tap's row alone, and the widths enter
//    the lengths as a sum.
// 3. Refusals, from stub circuit tables: each bad table is refused with its own text, and the nearest good one is taken.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "circuit.hpp"
#include "lookup.hpp"
#include "seal_layout.hpp"

using namespace bx;

static long failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures++ < 20) {                        \
                printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

// host entries of the built-in tables (the library's own tables stand next to their device stages)
static const bx_circuit_ops SYNTH = {nullptr, "synthetic (host entries only)", synth_normalize, synth_taps, synth_n_globals, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr, synthetic_constraints_at, nullptr, nullptr};
static const bx_circuit_ops LOOKUP = {nullptr, "lookup (host entries only)", lookup_normalize, lookup_taps, lookup_n_globals, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, lookup_constraints_at, nullptr, nullptr};

// ---- 1. the oracle's seals ---------------------------------------------------------------------------------------------------
static int oracle_cases(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) {
        printf("cannot open %s\n", path);
        return -1;
    }
    int cases = 0;
    unsigned po2, wc, wd, wa, rounds, hdr[BX_SEAL_HEADER_WORDS];
    unsigned long len;
    while (fscanf(f, " %u %u %u %u %u %lu %u %u %u %u %u %u", &po2, &wc, &wd, &wa, &rounds, &len, &hdr[0], &hdr[1], &hdr[2], &hdr[3], &hdr[4], &hdr[5]) == 12) {
        bx_segment_params shape{po2, wc, wd, wa, 0, 0};
        const char* e = synth_normalize(nullptr, &shape);
        CHECK(!e, "%s", e);
        const SealLayout L = seal_layout(shape, &SYNTH);
        CHECK(!L.error, "2^%u %u-%u-%u: %s", po2, wc, wd, wa, L.error);
        if (e || L.error) continue;
        CHECK(L.seal_words == len, "2^%u %u-%u-%u: %zu words laid out, the oracle's seal has %lu", po2, wc, wd, wa, L.seal_words, len);
        CHECK(L.queries_at + BX_QUERIES * L.per_query == L.seal_words, "2^%u %u-%u-%u: queries at %zu, %zu words each", po2, wc, wd, wa, L.queries_at, L.per_query);
        CHECK(L.rounds.size() == rounds, "2^%u: %zu FRI rounds", po2, L.rounds.size());
        const unsigned mine[BX_SEAL_HEADER_WORDS] = {L.shape.po2, L.shape.w_code, L.shape.w_data, L.shape.w_accum, L.shape.cons_terms, L.shape.cons_degree};
        CHECK(!memcmp(mine, hdr, sizeof hdr), "2^%u %u-%u-%u: the oracle's header is %u %u %u %u %u %u", po2, wc, wd, wa, hdr[0], hdr[1], hdr[2], hdr[3], hdr[4], hdr[5]);
        ++cases;
    }
    fclose(f);
    return cases;
}

// ---- 2. invariants -----------------------------------------------------------------------------------------------------------
static void check_tree(const TreeGeom& t, size_t rows, size_t cols) {
    CHECK(t.rows == rows && t.cols == cols && ((size_t)1 << t.layers) == rows, "tree of %zu x %zu: %zu x %zu, %u layers", rows, cols, t.rows, t.cols, t.layers);
    CHECK(t.top_layer < t.layers && t.top_size() <= BX_QUERIES, "top layer %u of %u", t.top_layer, t.layers);
    CHECK(t.top_layer + 1 == t.layers || 2 * t.top_size() > BX_QUERIES, "top layer %u of %u is not the deepest", t.top_layer, t.layers);
    CHECK(t.depth() == t.layers - t.top_layer && t.query_words() == cols + 8 * (size_t)(t.layers - t.top_layer), "opening of %zu words", t.query_words());
}

static void check_layout(const SealLayout& L, const bx_circuit_ops* circ) {
    const bx_segment_params& s = L.shape;
    const size_t N = (size_t)1 << s.po2;
    const uint32_t widths[4] = {s.w_code, s.w_data, s.w_accum, BX_CHECK_SIZE};
    CHECK(L.N == N && !memcmp(L.widths, widths, sizeof widths), "N %zu", L.N);
    // tap sets, combos, tap counts
    CHECK(L.n_combos == L.n_trace_combos + 1 && L.combo_backs.size() == L.n_combos && L.n_combos <= BX_MAX_COMBOS, "%zu combos", L.n_combos);
    CHECK(L.combo_backs.back() == std::vector<uint32_t>{0}, "the check combo is {0}");
    size_t div = 1, tap = 0;
    for (size_t id = 0; id < L.n_trace_combos; ++id) {
        div += L.combo_backs[id].size();
        for (size_t j = 0; j < id; ++j) CHECK(L.combo_backs[j] != L.combo_backs[id], "combos %zu and %zu hold the same tap set", j, id);
    }
    CHECK(L.n_div == div, "n_div %zu, 1 + the trace combos' taps = %zu", L.n_div, div);
    CHECK(L.tap_first[0] == 0, "tap_first[0] %zu", L.tap_first[0]);
    size_t next_new = 0;  // combos are numbered in order of first appearance
    for (int g = 0; g < 4; ++g) {
        CHECK(L.combo[g].size() == widths[g], "group %d: %zu combo ids", g, L.combo[g].size());
        CHECK(L.tap_first[g] == tap, "tap_first[%d] %zu, counted %zu", g, L.tap_first[g], tap);
        for (uint32_t col = 0; col < widths[g] && tap < L.tap_which.size(); ++col) {
            uint32_t bk[BX_MAX_TAPS] = {0};
            const uint32_t k = g < 3 ? circ->taps(circ->user, &s, g, col, bk) : 1;
            const uint32_t id = L.combo[g][col];
            if (g < 3 && id == next_new) ++next_new;
            CHECK(g < 3 ? id < next_new : id == L.n_trace_combos, "group %d column %u: combo %u", g, col, id);
            if (id >= L.n_combos) return;
            const std::vector<uint32_t>& B = L.backs(g, col);
            CHECK(&B == &L.combo_backs[id] && B.size() == k && !memcmp(B.data(), bk, 4 * (size_t)k), "group %d column %u: combo %u does not hold its tap set", g, col, id);
            for (uint32_t t = 0; t < k && tap < L.tap_which.size(); ++t, ++tap) CHECK(L.tap_which[tap] == col, "tap %zu is of column %u", tap, L.tap_which[tap]);
        }
        CHECK(L.tap_first[g + 1] >= L.tap_first[g], "tap_first is not monotone at %d", g);
    }
    CHECK(next_new == L.n_trace_combos, "%zu trace combos, %zu in use", L.n_trace_combos, next_new);
    CHECK(tap == L.total_taps && L.tap_which.size() == L.total_taps && L.tap_first[4] == L.total_taps, "%zu taps counted, total_taps %zu", tap, L.total_taps);
    CHECK(L.n_globals == (circ->n_globals ? circ->n_globals(circ->user, &s) : 0) && L.n_globals <= BX_MAX_GLOBALS, "%u public words", L.n_globals);
    // trees and FRI rounds
    size_t tops = 0, per_query = 0, size = N;
    for (int g = 0; g < 4; ++g) check_tree(L.trees[g], 4 * N, widths[g]);
    for (const SealLayout::Round& r : L.rounds) {
        CHECK(r.size == size && size > BX_FRI_MIN_DEGREE, "round of %zu, %zu are left", r.size, size);
        check_tree(r.tree, 4 * size / 16, 64);
        size /= 16;
    }
    CHECK(L.final_size == size && L.final_size <= BX_FRI_MIN_DEGREE && L.final_size >= 1, "final size %zu", L.final_size);
    CHECK(L.n_trees() == 4 + L.rounds.size() && L.query_words.size() == L.n_trees() && L.query_off.size() == L.n_trees() + 1, "%zu trees", L.n_trees());
    if (L.query_words.size() != L.n_trees() || L.query_off.size() != L.n_trees() + 1) return;
    for (size_t t = 0; t < L.n_trees(); ++t) {
        const TreeGeom& tr = L.tree(t);
        CHECK(&tr == (t < 4 ? &L.trees[t] : &L.rounds[t - 4].tree), "tree %zu", t);
        CHECK(L.query_off[t] == per_query && L.query_words[t] == tr.query_words(), "tree %zu: opening of %zu words at %zu", t, L.query_words[t], L.query_off[t]);
        tops += 8 * tr.top_size();
        per_query += tr.cols + 8 * (size_t)(tr.layers - tr.top_layer);
    }
    CHECK(L.per_query == per_query && L.query_off.back() == per_query, "per_query %zu, summed %zu", L.per_query, per_query);
    const size_t front = BX_SEAL_HEADER_WORDS + L.n_globals + tops + 4 * tap + 4 * size;
    CHECK(L.queries_at == front && L.seal_words == front + BX_QUERIES * per_query, "queries at %zu of %zu, summed %zu and %zu", L.queries_at, L.seal_words, front,
          front + BX_QUERIES * per_query);
}

static long invariants() {
    static const uint32_t W[] = {1, 2, 16, 256, 65535};
    const uint32_t WIDE = 65535;
    long layouts = 0;
    for (uint32_t po2 = 9; po2 <= 24; ++po2)
        for (uint32_t wc : W)
            for (uint32_t wd : W)
                for (uint32_t wa : W)
                    for (const bx_circuit_ops* circ : {&SYNTH, &LOOKUP}) {
                        const int wide = (wc == WIDE) + (wd == WIDE) + (wa == WIDE);
                        if (wide != 0 && wide != 3 && po2 != 9 && po2 != 24) continue;
                        bx_segment_params shape{po2, wc, wd, wa, 0, 0};
                        if (circ->normalize(circ->user, &shape)) {
                            CHECK(circ == &LOOKUP, "the synthetic circuit refuses 2^%u %u-%u-%u", po2, wc, wd, wa);
                            continue;  // the lookup circuit takes the shapes that hold 1 .. 63 value columns
                        }
                        const SealLayout L = seal_layout(shape, circ);
                        CHECK(!L.error, "%s 2^%u %u-%u-%u: %s", circ->name, po2, wc, wd, wa, L.error);
                        if (L.error) continue;
                        const long before = failures;
                        check_layout(L, circ);
                        if (failures != before && before < 20) printf("  (%s 2^%u %u-%u-%u)\n", circ->name, po2, wc, wd, wa);
                        ++layouts;
                    }
    return layouts;
}

// ---- 3. refusals -------------------------------------------------------------------------------------------------------------
enum Stub { ZERO_ENTRIES, NINE_ENTRIES, EIGHT_ENTRIES, FIRST_NOT_ZERO, NOT_INCREASING, REPEATED, ENTRY_IS_N, ENTRY_BELOW_N, DISTINCT_SETS };
struct StubUser {
    Stub kind;
    uint32_t globals;
};
static uint32_t stub_taps(void* user, const bx_segment_params* s, int group, uint32_t col, uint32_t* out) {
    for (uint32_t t = 0; t < BX_MAX_TAPS; ++t) out[t] = t;  // never more than the BX_MAX_TAPS words a caller provides
    if (group != 1) return 1;
    switch (((const StubUser*)user)->kind) {
    case ZERO_ENTRIES: return col == 2 ? 0 : 1;
    case NINE_ENTRIES: return col == 2 ? 9 : 1;
    case EIGHT_ENTRIES: return col == 2 ? 8 : 1;
    case FIRST_NOT_ZERO: out[0] = col == 2 ? 1 : 0; return 1;
    case NOT_INCREASING: if (col == 2) out[1] = 3, out[2] = 2; return 3;
    case REPEATED: if (col == 2) out[2] = 1; return 3;
    case ENTRY_IS_N: out[1] = 1u << s->po2; return 2;
    case ENTRY_BELOW_N: out[1] = (1u << s->po2) - 1; return 2;
    case DISTINCT_SETS: out[1] = 1 + col; return 2;  // {0, 1 + col}: as many sets as data columns, none of them the other groups' {0}
    }
    return 1;
}
static uint32_t stub_globals(void* user, const bx_segment_params*) { return ((const StubUser*)user)->globals; }

static void expect(Stub kind, uint32_t w_data, uint32_t globals, const char* refusal) {
    StubUser user{kind, globals};
    const bx_circuit_ops ops = {&user, "stub", nullptr, stub_taps, stub_globals, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const bx_segment_params shape{9, 3, w_data, 2, 0, 0};
    const SealLayout L = seal_layout(shape, &ops);
    if (refusal) {
        CHECK(L.error && !strcmp(L.error, refusal), "stub %d, %u data columns, %u public words: '%s', expected '%s'", (int)kind, w_data, globals, L.error ? L.error : "(taken)", refusal);
    } else {
        CHECK(!L.error, "stub %d, %u data columns, %u public words: %s", (int)kind, w_data, globals, L.error);
        if (!L.error) check_layout(L, &ops);
    }
}

static void refusals() {
    const char* const ENTRIES = "a tap set has 1..8 entries and starts with 0";
    const char* const INCREASING = "tap sets are strictly increasing";
    expect(ZERO_ENTRIES, 4, 0, ENTRIES);
    expect(NINE_ENTRIES, 4, 0, ENTRIES);
    expect(EIGHT_ENTRIES, 4, 0, nullptr);
    expect(FIRST_NOT_ZERO, 4, 0, ENTRIES);
    expect(NOT_INCREASING, 4, 0, INCREASING);
    expect(REPEATED, 4, 0, INCREASING);
    expect(ENTRY_IS_N, 4, 0, INCREASING);
    expect(ENTRY_BELOW_N, 4, 0, nullptr);
    // the other groups' {0} and one set per data column: 15 distinct sets and the check group's own combo are BX_MAX_COMBOS, 16 are
    // one too many
    expect(DISTINCT_SETS, 14, 0, nullptr);
    expect(DISTINCT_SETS, 15, 0, "too many distinct tap sets");
    expect(DISTINCT_SETS, 300, 0, "too many distinct tap sets");
    expect(EIGHT_ENTRIES, 4, BX_MAX_GLOBALS, nullptr);
    expect(EIGHT_ENTRIES, 4, BX_MAX_GLOBALS + 1, "too many public words");
    // a table that is refused for its tap sets is refused for them first, as the callers did before the layout existed
    expect(NINE_ENTRIES, 4, BX_MAX_GLOBALS + 1, ENTRIES);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: seal_layout_check <cases.txt>\n");
        return 2;
    }
    const int cases = oracle_cases(argv[1]);
    if (cases <= 0) return 1;
    const long layouts = invariants();
    refusals();
    printf("%d oracle seals compared, %ld layouts checked, %ld failures\n", cases, layouts, failures);
    if (failures) return 1;
    printf("seal_layout_check ok\n");
    return 0;
}
