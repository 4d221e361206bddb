// lookup.hpp — shape of the lookup circuit (include/bx_lookup.h, "The lookup circuit", is the normative text): how many value
// columns a shape holds, the limb width, which columns are opened one row back, what a code cell is.  Shared by the device stages
// (lookup.hip), the verifier-side constraint evaluation (lookup_host.cpp) and the host control IDs (control_id.cpp); host-only
// builds of the verifier need nothing else of the circuit.  tests/lookup_ref.py restates the same rules independently.
#pragma once
#include "../../include/bx_lookup.h"
#include "circuit.hpp"

namespace bx {

constexpr uint64_t LOOKUP_CODE_SEED = 0x4C4F4F4B55502121ull;  // "LOOKUP!!"

struct Lookup {
    uint32_t po2, wc, wd, wa;
    uint32_t V, S, b, B;  // value columns, sequences 2V + 1, limb bits, table size
    Lookup() = default;
    Lookup(uint32_t po2_, uint32_t w_code, uint32_t w_data, uint32_t w_accum) : po2(po2_), wc(w_code), wd(w_data), wa(w_accum) {
        const uint32_t vd = wd ? (wd - 1) / 3 : 0, e = wa / 4, va = e ? (e - 1) / 2 : 0;
        V = vd < va ? vd : va;
        S = 2 * V + 1;
        b = po2 - 1 < BX_LOOKUP_MAX_LIMB_BITS ? po2 - 1 : BX_LOOKUP_MAX_LIMB_BITS;
        B = 1u << b;
    }
    BX_CIRC_HD uint32_t zk_rows() const { return ((1u << po2) >> 2) < 1994u ? ((1u << po2) >> 2) : 1994u; }
    BX_CIRC_HD uint32_t active_rows() const { return (1u << po2) - zk_rows(); }
    BX_CIRC_HD uint32_t limb_col(uint32_t s) const { return 3 * (s >> 1) + 1 + (s & 1u); }  // data column of sequence s < 2V
    BX_CIRC_HD uint32_t mult_col() const { return 3 * V; }
    size_t constraints() const { return 3 * (size_t)V + 4; }
};

inline Lookup lookup_of(const bx_segment_params* s) { return Lookup(s->po2, s->w_code, s->w_data, s->w_accum); }
inline const char* lookup_normalize(void*, bx_segment_params* s) {
    if (!s) return "circuit: null shape";
    if (s->cons_terms || s->cons_degree) return "lookup circuit: cons_terms and cons_degree are unused and must be 0";
    if (s->po2 < 9 || s->po2 > 24) return "lookup circuit: po2 must be in [9, 24]";
    if (s->w_code < 3) return "lookup circuit: w_code must be at least 3 (first, last, the table)";
    const Lookup lk = lookup_of(s);
    if (lk.V == 0) return "lookup circuit: no value column fits (w_data >= 4 and w_accum >= 12 are needed)";
    if (lk.V > BX_LOOKUP_MAX_VALUES) return "lookup circuit: more than 63 value columns";
    return nullptr;
}
inline uint32_t lookup_taps(void*, const bx_segment_params* s, int group, uint32_t col, uint32_t* backs_out /* BX_MAX_TAPS */) {
    backs_out[0] = 0;
    if (group == 2 && col < 4 * lookup_of(s).S) {
        backs_out[1] = 1;
        return 2;
    }
    return 1;
}
inline uint32_t lookup_n_globals(void*, const bx_segment_params*) { return 2; }
// cell (col, row) of the code group: first, last, the table, control words
BX_CIRC_HD inline uint32_t lookup_code_cell(const Lookup& lk, uint32_t col, uint32_t row) {
    constexpr uint32_t ONE = 268435454u;  // Montgomery form of 1
    if (col == 0) return row == 0 ? ONE : 0u;
    if (col == 1) return row == lk.active_rows() - 1 ? ONE : 0u;
    if (col == 2) return row < lk.B ? (uint32_t)(((uint64_t)row << 32) % 2013265921u) : 0u;  // the value r as a Montgomery word
    return synth_word(LOOKUP_CODE_SEED, col, row);
}
// verifier side of the code-group binding (control_id.cpp): the cached host computation, Poseidon2
const char* lookup_check_code(void*, const bx_segment_params* s, const uint32_t root[8]);
const char* lookup_check_code_suite(const bx_segment_params* s, const uint32_t root[8], int suite);
// sum_i poly_mix^i C_i from the tap values (lookup_host.cpp)
const char* lookup_constraints_at(void*, const bx_segment_params* shape, const bx_tap_reader* taps, const uint32_t poly_mix[4], const uint32_t mix[4],
                                  const uint32_t* globals, uint32_t out[4]);

}  // namespace bx
