// trace_layout.hpp — a compiled trace layout (include/bx_layout.h, "Trace layouts", is the normative text): the description as
// bx_trace_layout_create checked it, what a code cell is, and the per-column table the place kernel walks.  Shared by the host half
// (trace_layout_host.cpp: create, the host fills, the base table's host entries), the control IDs (control_id.cpp) and the device half
// (trace_layout.hip).  tests/trace_layout_ref.py restates the same rules independently.
#pragma once
#include <array>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/bx_layout.h"
#include "circuit.hpp"

namespace bx {

// rows of a shape: Z = min(noise_rows, N / 4), A = N - Z
BX_CIRC_HD inline uint32_t layout_active_rows(uint32_t po2, uint32_t noise_rows) {
    const uint32_t n = 1u << po2, z = (n >> 2) < noise_rows ? (n >> 2) : noise_rows;
    return n - z;
}
// the Montgomery word of a value below 2^32 (x * 2^32 mod P): one 64-bit remainder, so that host-only users need no fp.hpp
BX_CIRC_HD inline uint32_t layout_encode(uint32_t x) { return (uint32_t)(((uint64_t)x << 32) % 2013265921u); }

// cell (col, row) of the code group from the column's (kind, a, b); `act` = A of the shape, `n` = N.  LAST / ACTIVE with a >= A
// never get here (layout_check_shape).
BX_CIRC_HD inline uint32_t layout_code_cell(const bx_layout_code_col& k, const uint32_t* table, uint32_t col, uint32_t row, uint32_t n, uint32_t act) {
    constexpr uint32_t ONE = 268435454u;  // Montgomery form of 1
    switch (k.kind) {
    case BX_LAYOUT_CONST: return layout_encode(k.a);
    case BX_LAYOUT_FIRST: return row == 0 ? ONE : 0u;
    case BX_LAYOUT_LAST: return row == act - 1u - k.a ? ONE : 0u;
    case BX_LAYOUT_ACTIVE: return row < act - k.a ? ONE : 0u;
    case BX_LAYOUT_ROW: return row < (k.a && k.a < n ? k.a : n) ? layout_encode(row) : 0u;
    case BX_LAYOUT_PERIODIC: return layout_encode(table[k.b + (row & ((1u << k.a) - 1u))]);
    default: return synth_word((uint64_t)k.a | ((uint64_t)k.b << 32), col, row);  // BX_LAYOUT_WORD
    }
}

// what the place kernel knows of one data column: the value is (record[word] >> shift) & mask below R and `pad` (a Montgomery word)
// on [R, A).  A column without a field is the entry {0, 0, 0, 0}: the value 0 everywhere below A.
struct LayoutColumn {
    uint32_t word, shift, mask, pad;
};

}  // namespace bx

struct bx_trace_layout {
    std::vector<bx_layout_code_col> code;
    std::vector<uint32_t> table;
    std::vector<bx_layout_field> fields;
    uint32_t stride = 1, noise_rows = 0, n_globals = 0;
    uint32_t min_w_data = 0;  // the largest field column + 1
    bx_circuit_ops ops{};     // the base table: create sets the host entries and, through g_layout_device_entries, the device ones
    // host-computed control IDs, per (po2, suite)
    mutable std::mutex mu;
    mutable std::map<std::pair<uint32_t, int>, std::array<uint32_t, 8>> ids;

    // the per-column table of a data group of w_data >= min_w_data columns
    std::vector<bx::LayoutColumn> columns(uint32_t w_data) const {
        std::vector<bx::LayoutColumn> t(w_data, bx::LayoutColumn{0u, 0u, 0u, 0u});
        for (const bx_layout_field& f : fields)
            t[f.col] = bx::LayoutColumn{f.word, f.shift, (uint32_t)((1ull << f.bits) - 1ull), bx::layout_encode(f.pad)};
        return t;
    }
};

namespace bx {
// The device entries of a layout's base table (create, destroy, code_group, witgen, accumulate, set_noise_seed) are trace_layout.hip's:
// it registers the function that fills them in.  A host-only build (the stand-alone checker) has none, and its tables have none.
extern void (*g_layout_device_entries)(bx_circuit_ops*);
// LAST / ACTIVE against the shape's A; NULL or a message in `err`
const char* layout_check_shape(const bx_trace_layout* l, uint32_t po2, const char* who, char* err, size_t err_len);
// the payload of a segment against the layout: its record count R, or why witgen refuses it
const char* layout_check_payload(const bx_trace_layout* l, uint32_t po2, size_t segment_len, const char* who, uint32_t* records, char* err, size_t err_len);
// control_id.cpp: the Merkle root of the layout's committed code group, by the definition-level host path of the built-in circuits
const char* layout_host_control_id(const bx_trace_layout* l, uint32_t po2, int suite, uint32_t out[8]);
}  // namespace bx
