// seal_layout.hpp — where every word of a seal stands, decided on the host from the shape and the circuit's tap sets (DESIGN.md §1
// "The layout").
//
// Host-only and integers only: no HIP header, no context, no pointer to device memory, no field arithmetic, no transcript.
// seal_layout() maps (normalised shape, circuit table) to the tap set and DEEP combo of every column, the tap counts, the geometry of
// the four trace trees and of every FRI round's tree, the words of one query and the length of the seal — or to the text of a circuit
// table that is refused.  The prover (prover.hip) allocates and proves by it, the verifier (verify.cpp) reads a seal by it; neither
// derives any of these numbers again.  Header-only: the verifier also builds with plain g++ from a list of source files.  The
// restatements that keep sharing it honest share nothing with it: oracle/, tests/plain_hal_prover.c and the reference models under
// tests/; tests/seal_layout_check.cpp holds it against the oracle's seals and walks every size without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/bx_circuit.h"
#include "../../include/bx_hal.h"

namespace bx {

// MerkleTreeProver / MerkleTreeVerifier: the layer a seal carries in full, the deepest one with at most BX_QUERIES nodes.
inline unsigned top_layer_of(unsigned layers) {
    unsigned top = 0;
    while (top + 1 < layers && (2u << top) <= BX_QUERIES) ++top;
    return top;
}

// A Merkle tree over the rows (a power of two) of a rows x cols matrix: what of it a seal carries.
struct TreeGeom {
    size_t rows = 0, cols = 0;
    unsigned layers = 0, top_layer = 0;
    TreeGeom() = default;
    TreeGeom(size_t rows_, size_t cols_) : rows(rows_), cols(cols_) {
        while (((size_t)1 << layers) < rows) ++layers;
        top_layer = top_layer_of(layers);
    }
    size_t top_size() const { return (size_t)1 << top_layer; }       // digests written after the commit
    unsigned depth() const { return layers - top_layer; }            // siblings of one opening (those below the top layer)
    size_t query_words() const { return cols + 8 * (size_t)depth(); }  // one opening: the row, then the path
};

struct SealLayout {
    const char* error = nullptr;  // a refused circuit table (the caller puts its own prefix in front); nothing else is valid then
    bx_segment_params shape{};    // as given: range-checked and normalised by the caller
    size_t N = 0;                 // trace rows, 2^po2
    uint32_t widths[4] = {0, 0, 0, 0};  // code, data, accum, check
    // Every column is opened at Z and at the rows back its tap set lists (bx_circuit.h); columns with the same set share a DEEP
    // combination polynomial ("combo").  Combos are numbered in order of first appearance over code, data, accum; the check group's
    // own combo {0} comes last (a trace column opened at Z alone is in a trace combo {0}, not in that one).
    std::vector<uint32_t> combo[4];                  // per group: the combo of each column
    std::vector<std::vector<uint32_t>> combo_backs;  // per combo: its tap set, backs[0] == 0, strictly increasing
    size_t n_trace_combos = 0, n_combos = 0;
    const std::vector<uint32_t>& backs(int g, uint32_t col) const { return combo_backs[combo[g][col]]; }
    // tap evaluations (ext elements of coeff_u), column by column, group by group
    size_t tap_first[5] = {0, 0, 0, 0, 0};  // first tap evaluation of each group; tap_first[4] == total_taps
    size_t total_taps = 0;
    std::vector<uint32_t> tap_which;  // column (within its group) of every tap evaluation
    size_t n_div = 0;                 // DEEP divisions: one per tap point of every combo
    uint32_t n_globals = 0;           // public words of the statement (bx_circuit_ops::n_globals)
    TreeGeom trees[4];                // over the 4N evaluations of each group
    struct Round {
        size_t size = 0;  // ext coefficients entering the round
        TreeGeom tree;    // 4 * size / BX_FRI_FOLD rows of BX_FRI_FOLD ext evaluations
    };
    std::vector<Round> rounds;
    size_t final_size = 0;  // ext coefficients of the final polynomial
    // a query opens every tree once: the four groups, then the rounds
    size_t n_trees() const { return 4 + rounds.size(); }
    const TreeGeom& tree(size_t t) const { return t < 4 ? trees[t] : rounds[t - 4].tree; }
    std::vector<size_t> query_words;  // per tree: words of one opening
    std::vector<size_t> query_off;    // per tree: words of one query in front of its opening; query_off[n_trees()] == per_query
    size_t per_query = 0;
    size_t queries_at = 0;  // word offset of query 0
    size_t seal_words = 0;  // header | public words | 4 trace tops | coeff_u | FRI tops | final coefficients | BX_QUERIES queries
};

// `shape`: po2 in [9, 24], widths in [1, 65535], knobs normalised by the circuit (the callers' checks: their texts differ).
inline SealLayout seal_layout(const bx_segment_params& shape, const bx_circuit_ops* circ) {
    SealLayout L;
    L.shape = shape;
    L.N = (size_t)1 << shape.po2;
    const uint32_t widths[4] = {shape.w_code, shape.w_data, shape.w_accum, BX_CHECK_SIZE};
    std::copy(widths, widths + 4, L.widths);
    for (int g = 0; g < 3; ++g) {
        L.combo[g].resize(widths[g]);
        for (uint32_t col = 0; col < widths[g]; ++col) {
            uint32_t bk[BX_MAX_TAPS];
            const uint32_t k = circ->taps(circ->user, &L.shape, g, col, bk);
            if (!(k >= 1 && k <= BX_MAX_TAPS && bk[0] == 0)) return L.error = "a tap set has 1..8 entries and starts with 0", L;
            for (uint32_t t = 1; t < k; ++t)
                if (!(bk[t] > bk[t - 1] && bk[t] < L.N)) return L.error = "tap sets are strictly increasing", L;
            size_t id = 0;
            while (id < L.combo_backs.size() && !(L.combo_backs[id].size() == k && std::equal(bk, bk + k, L.combo_backs[id].begin()))) ++id;
            if (id == L.combo_backs.size()) L.combo_backs.emplace_back(bk, bk + k);
            L.combo[g][col] = (uint32_t)id;
            L.total_taps += k;
        }
    }
    if (L.combo_backs.size() + 1 > BX_MAX_COMBOS) return L.error = "too many distinct tap sets", L;
    L.n_trace_combos = L.combo_backs.size();
    L.n_combos = L.n_trace_combos + 1;
    L.combo_backs.push_back({0});
    L.combo[3].assign(BX_CHECK_SIZE, (uint32_t)L.n_trace_combos);
    L.total_taps += BX_CHECK_SIZE;
    for (const auto& b : L.combo_backs) L.n_div += b.size();
    L.n_globals = circ->n_globals ? circ->n_globals(circ->user, &L.shape) : 0;
    if (L.n_globals > BX_MAX_GLOBALS) return L.error = "too many public words", L;

    size_t words = BX_SEAL_HEADER_WORDS + (size_t)L.n_globals, tap = 0;
    L.tap_which.resize(L.total_taps);
    for (int g = 0; g < 4; ++g) {
        for (uint32_t col = 0; col < widths[g]; ++col)
            for (size_t k = L.backs(g, col).size(); k; --k) L.tap_which[tap++] = col;
        L.tap_first[g + 1] = tap;
        L.trees[g] = TreeGeom(BX_INV_RATE * L.N, widths[g]);
        words += 8 * L.trees[g].top_size();
    }
    words += 4 * L.total_taps;
    size_t size = L.N;
    for (; size > BX_FRI_MIN_DEGREE; size /= BX_FRI_FOLD) {
        L.rounds.push_back({size, TreeGeom(BX_INV_RATE * size / BX_FRI_FOLD, 4 * BX_FRI_FOLD)});
        words += 8 * L.rounds.back().tree.top_size();
    }
    L.final_size = size;
    words += 4 * L.final_size;
    L.query_off.push_back(0);
    for (size_t t = 0; t < L.n_trees(); ++t) {
        L.query_words.push_back(L.tree(t).query_words());
        L.query_off.push_back(L.query_off[t] + L.query_words[t]);
    }
    L.per_query = L.query_off.back();
    L.queries_at = words;
    L.seal_words = words + BX_QUERIES * L.per_query;
    return L;
}

}  // namespace bx
