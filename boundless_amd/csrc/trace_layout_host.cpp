// trace_layout_host.cpp — host half of trace layouts (include/bx_layout.h): the create rules, the info getter, the two host fills, the
// control ID, and the host entries of the base table (normalize, taps, n_globals, check_code, and the two refusals that say a layout
// is a base and not a circuit).  Plain C++, no HIP header: tests/trace_layout_check.cpp compiles it as a stand-alone program under the
// sanitizers, together with control_id.cpp (the definition-level commitment of a code group).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>

#include "trace_layout.hpp"

namespace bx {
void (*g_layout_device_entries)(bx_circuit_ops*) = nullptr;  // set by trace_layout.hip where the library has its device half
namespace {
constexpr uint32_t FIELD_P = 2013265921u;
thread_local char g_err[384];

#define BX_LAYOUT_REFUSE(...)                                \
    do {                                                      \
        snprintf(g_err, sizeof g_err, __VA_ARGS__);           \
        return g_err;                                         \
    } while (0)

// the thirteen rules of bx_trace_layout_create, in the header's order: each over the whole description before the next
const char* check_desc(const bx_trace_layout_desc& d) {
    for (uint32_t c = 0; c < d.n_code; ++c)
        if (d.code[c].kind > BX_LAYOUT_WORD) BX_LAYOUT_REFUSE("trace_layout: code column %u: unknown kind %u", c, d.code[c].kind);
    for (uint32_t c = 0; c < d.n_code; ++c) {
        const bx_layout_code_col& k = d.code[c];
        if (k.kind == BX_LAYOUT_CONST && k.a >= FIELD_P) BX_LAYOUT_REFUSE("trace_layout: code column %u: CONST value %u is not below P", c, k.a);
        if (k.kind == BX_LAYOUT_PERIODIC && k.a > BX_LAYOUT_MAX_PERIOD_BITS)
            BX_LAYOUT_REFUSE("trace_layout: code column %u: PERIODIC period 2^%u is above 2^12", c, k.a);
    }
    for (uint32_t c = 0; c < d.n_code; ++c) {
        const bx_layout_code_col& k = d.code[c];
        if (k.kind == BX_LAYOUT_PERIODIC && (uint64_t)k.b + (1ull << k.a) > d.n_table)
            BX_LAYOUT_REFUSE("trace_layout: code column %u: PERIODIC window [%u, %llu) is outside the table of %u values", c, k.b,
                             (unsigned long long)((uint64_t)k.b + (1ull << k.a)), d.n_table);
    }
    for (uint32_t i = 0; i < d.n_table; ++i)
        if (d.table[i] >= FIELD_P) BX_LAYOUT_REFUSE("trace_layout: table value %u (%u) is not below P", i, d.table[i]);
    if (d.stride == 0 || d.stride > BX_LAYOUT_MAX_STRIDE) BX_LAYOUT_REFUSE("trace_layout: stride %u is not in 1 .. 128", d.stride);
    for (uint32_t i = 0; i < d.n_fields; ++i)
        if (d.fields[i].word >= d.stride) BX_LAYOUT_REFUSE("trace_layout: field %u: word %u is not below the stride %u", i, d.fields[i].word, d.stride);
    for (uint32_t i = 0; i < d.n_fields; ++i)
        if (d.fields[i].bits == 0 || d.fields[i].bits > BX_LAYOUT_MAX_FIELD_BITS) BX_LAYOUT_REFUSE("trace_layout: field %u: bits %u is not in 1 .. 30", i, d.fields[i].bits);
    for (uint32_t i = 0; i < d.n_fields; ++i)
        if ((uint64_t)d.fields[i].shift + d.fields[i].bits > 32)
            BX_LAYOUT_REFUSE("trace_layout: field %u: shift %u + bits %u is above 32", i, d.fields[i].shift, d.fields[i].bits);
    for (uint32_t i = 0; i < d.n_fields; ++i)
        if (d.fields[i].pad >> d.fields[i].bits) BX_LAYOUT_REFUSE("trace_layout: field %u: pad %u is not below 2^%u", i, d.fields[i].pad, d.fields[i].bits);
    {
        // the first field, in list order, whose column an earlier field names
        std::vector<std::pair<uint32_t, uint32_t>> by_col(d.n_fields);  // (column, field)
        for (uint32_t i = 0; i < d.n_fields; ++i) by_col[i] = {d.fields[i].col, i};
        std::sort(by_col.begin(), by_col.end());
        uint32_t second = UINT32_MAX;
        for (uint32_t i = 1; i < d.n_fields; ++i)  // sorted by (column, field): an entry behind one of its own column is a repeat
            if (by_col[i].first == by_col[i - 1].first && by_col[i].second < second) second = by_col[i].second;
        if (second != UINT32_MAX) {
            uint32_t first = 0;
            while (d.fields[first].col != d.fields[second].col) ++first;
            BX_LAYOUT_REFUSE("trace_layout: field %u: column %u is named a second time (first by field %u)", second, d.fields[second].col, first);
        }
    }
    if (d.n_code == 0 || d.n_code >= 65536) BX_LAYOUT_REFUSE("trace_layout: n_code %u is not in 1 .. 65535", d.n_code);
    for (uint32_t i = 0; i < d.n_fields; ++i)
        if (d.fields[i].col >= 65535) BX_LAYOUT_REFUSE("trace_layout: field %u: column %u is not below 65535", i, d.fields[i].col);
    if (d.n_globals > BX_MAX_GLOBALS) BX_LAYOUT_REFUSE("trace_layout: n_globals %u is above BX_MAX_GLOBALS = 64", d.n_globals);
    return nullptr;
}

int suite_of(const char* hashfn) {  // the names of hash_suite.hpp
    if (hashfn && strcmp(hashfn, "poseidon2") == 0) return 0;
    if (hashfn && strcmp(hashfn, "sha-256") == 0) return 1;
    return -1;
}

// the cached control ID of (layout, po2, suite)
const char* cached_id(const bx_trace_layout* l, uint32_t po2, int suite, uint32_t out[8]) {
    if (po2 < 9 || po2 > 24) return "bx_trace_layout_control_id_host: shape out of range (po2 in [9, 24])";
    if (const char* e = layout_check_shape(l, po2, "bx_trace_layout_control_id_host", g_err, sizeof g_err)) return e;
    const std::pair<uint32_t, int> key{po2, suite};
    {
        std::lock_guard<std::mutex> g(l->mu);
        auto it = l->ids.find(key);
        if (it != l->ids.end()) {
            memcpy(out, it->second.data(), 32);
            return nullptr;
        }
    }
    std::array<uint32_t, 8> d;
    if (const char* e = layout_host_control_id(l, po2, suite, d.data())) return e;
    std::lock_guard<std::mutex> g(l->mu);
    l->ids[key] = d;
    memcpy(out, d.data(), 32);
    return nullptr;
}

// ---- the host entries of the base table ----
const char* layout_normalize(void* user, bx_segment_params* s) {
    const bx_trace_layout* l = (const bx_trace_layout*)user;
    if (!s) return "circuit: null shape";
    if (s->cons_terms || s->cons_degree) return "trace layout: cons_terms and cons_degree are unused and must be 0";
    if (s->po2 < 1 || s->po2 > 24) return "trace layout: po2 must be in [1, 24]";
    if (s->w_code != l->code.size()) BX_LAYOUT_REFUSE("trace layout: w_code is %u, the layout has %zu code columns", s->w_code, l->code.size());
    if (s->w_data < l->min_w_data) BX_LAYOUT_REFUSE("trace layout: w_data is %u, a field names data column %u", s->w_data, l->min_w_data - 1);
    return layout_check_shape(l, s->po2, "trace layout", g_err, sizeof g_err);
}
uint32_t layout_taps(void*, const bx_segment_params*, int, uint32_t, uint32_t* backs_out) {
    backs_out[0] = 0;
    return 1;
}
uint32_t layout_n_globals(void* user, const bx_segment_params*) { return ((const bx_trace_layout*)user)->n_globals; }
constexpr const char* NOT_A_CIRCUIT =
    "trace layout: a layout is the base of a circuit, not a circuit: it has no constraints (give it a constraint program with bx_cons_circuit_create)";
const char* layout_eval_check(void*, void*, bx_ctx*, bx_buf, bx_buf, bx_buf, bx_buf, const uint32_t*, const uint32_t*, const uint32_t*) { return NOT_A_CIRCUIT; }
const char* layout_constraints_at(void*, const bx_segment_params*, const bx_tap_reader*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*) {
    return NOT_A_CIRCUIT;
}
const char* layout_check_code(void* user, const bx_segment_params* s, const uint32_t root[8]) {
    if (!s || !root) return "check_code: null argument";
    const bx_trace_layout* l = (const bx_trace_layout*)user;
    if (s->w_code != l->code.size()) return "the seal's w_code is not the layout's number of code columns";
    uint32_t id[8];
    try {
        if (const char* e = cached_id(l, s->po2, 0 /* Poseidon2: a table's check_code has no suite parameter */, id)) return e;
    } catch (...) {
        return "trace layout: check_code: out of host memory";
    }
    return memcmp(id, root, 32) == 0 ? nullptr : "the code group's root is not this layout's control ID for the shape (the seal was made with another code group)";
}
}  // namespace

const char* layout_check_shape(const bx_trace_layout* l, uint32_t po2, const char* who, char* err, size_t err_len) {
    const uint32_t act = layout_active_rows(po2, l->noise_rows);
    for (size_t c = 0; c < l->code.size(); ++c) {
        const bx_layout_code_col& k = l->code[c];
        if ((k.kind == BX_LAYOUT_LAST || k.kind == BX_LAYOUT_ACTIVE) && k.a >= act) {
            snprintf(err, err_len, "%s: code column %zu: %s with a = %u needs more than the %u active rows of po2 %u", who, c,
                     k.kind == BX_LAYOUT_LAST ? "LAST" : "ACTIVE", k.a, act, po2);
            return err;
        }
    }
    return nullptr;
}

const char* layout_check_payload(const bx_trace_layout* l, uint32_t po2, size_t segment_len, const char* who, uint32_t* records, char* err, size_t err_len) {
    if (segment_len < BX_SEGMENT_WIRE_BYTES) {
        snprintf(err, err_len, "%s: the segment is shorter than its 28-byte header", who);
        return err;
    }
    const size_t payload = segment_len - BX_SEGMENT_WIRE_BYTES, rec = 4 * (size_t)l->stride;
    if (payload % rec) {
        snprintf(err, err_len, "%s: the payload of %zu bytes is not a whole number of %zu-byte records (stride %u)", who, payload, rec, l->stride);
        return err;
    }
    const uint32_t act = layout_active_rows(po2, l->noise_rows);
    if (payload / rec > act) {
        snprintf(err, err_len, "%s: the payload holds %zu records, the trace has %u active rows", who, payload / rec, act);
        return err;
    }
    *records = (uint32_t)(payload / rec);
    return nullptr;
}
}  // namespace bx

extern "C" {

const char* bx_trace_layout_create(const bx_trace_layout_desc* desc, bx_trace_layout** out) try {
    using namespace bx;
    if (!desc || !out || (desc->n_code && !desc->code) || (desc->n_table && !desc->table) || (desc->n_fields && !desc->fields))
        return "bx_trace_layout_create: null argument";
    *out = nullptr;
    if (const char* e = check_desc(*desc)) return e;
    std::unique_ptr<bx_trace_layout> l(new bx_trace_layout());
    l->code.assign(desc->code, desc->code + desc->n_code);
    if (desc->n_table) l->table.assign(desc->table, desc->table + desc->n_table);
    if (desc->n_fields) l->fields.assign(desc->fields, desc->fields + desc->n_fields);
    l->stride = desc->stride;
    l->noise_rows = desc->noise_rows;
    l->n_globals = desc->n_globals;
    for (const bx_layout_field& f : l->fields) l->min_w_data = std::max(l->min_w_data, f.col + 1);
    l->ops.user = l.get();
    l->ops.name = "bx-trace-layout";
    l->ops.normalize = layout_normalize;
    l->ops.taps = layout_taps;
    l->ops.n_globals = layout_n_globals;
    l->ops.eval_check = layout_eval_check;
    l->ops.constraints_at = layout_constraints_at;
    l->ops.check_code = layout_check_code;
    if (g_layout_device_entries) g_layout_device_entries(&l->ops);
    *out = l.release();
    return nullptr;
} catch (...) {
    return "bx_trace_layout_create: out of host memory";
}

void bx_trace_layout_destroy(bx_trace_layout* layout) { delete layout; }

const bx_circuit_ops* bx_trace_layout_ops(bx_trace_layout* layout) { return layout ? &layout->ops : nullptr; }

const char* bx_trace_layout_info_get(const bx_trace_layout* l, bx_trace_layout_info* out) {
    if (!l || !out) return "bx_trace_layout_info_get: null argument";
    *out = bx_trace_layout_info{(uint32_t)l->code.size(), (uint32_t)l->table.size(), (uint32_t)l->fields.size(), l->stride, l->noise_rows, l->n_globals, l->min_w_data};
    return nullptr;
}

const char* bx_trace_layout_code_host(const bx_trace_layout* l, uint32_t po2, uint32_t* code_out) {
    using namespace bx;
    if (!l || !code_out) return "bx_trace_layout_code_host: null argument";
    if (po2 < 1 || po2 > 24) return "bx_trace_layout_code_host: po2 must be in [1, 24]";
    if (const char* e = layout_check_shape(l, po2, "bx_trace_layout_code_host", g_err, sizeof g_err)) return e;
    const uint32_t n = 1u << po2, act = layout_active_rows(po2, l->noise_rows);
    for (size_t c = 0; c < l->code.size(); ++c)
        for (uint32_t r = 0; r < n; ++r) code_out[c * n + r] = layout_code_cell(l->code[c], l->table.data(), (uint32_t)c, r, n, act);
    return nullptr;
}

const char* bx_trace_layout_data_host(const bx_trace_layout* l, uint32_t po2, const uint8_t* segment, size_t segment_len, const uint64_t* noise_seed,
                                      uint32_t* data_out, uint32_t w_data) try {
    using namespace bx;
    const char* who = "bx_trace_layout_data_host";
    if (!l || !segment || !data_out) return "bx_trace_layout_data_host: null argument";
    if (po2 < 1 || po2 > 24) return "bx_trace_layout_data_host: po2 must be in [1, 24]";
    if (w_data < l->min_w_data) BX_LAYOUT_REFUSE("%s: w_data is %u, a field names data column %u", who, w_data, l->min_w_data - 1);
    uint32_t records = 0;
    if (const char* e = layout_check_payload(l, po2, segment_len, who, &records, g_err, sizeof g_err)) return e;
    const auto le = [&](size_t at, int bytes) {
        uint64_t v = 0;
        for (int i = bytes - 1; i >= 0; --i) v = (v << 8) | segment[at + i];
        return v;
    };
    if (memcmp(segment, BX_SEGMENT_MAGIC, 8) != 0) BX_LAYOUT_REFUSE("%s: the segment does not start with \"BXSYNSEG\"", who);
    if ((uint32_t)le(16, 4) != po2) BX_LAYOUT_REFUSE("%s: the segment has po2 %u, the fill was asked for po2 %u", who, (uint32_t)le(16, 4), po2);
    const uint64_t seed = le(20, 8);
    const uint64_t nseed = (noise_seed ? *noise_seed : splitmix64(seed ^ 0x5A4B4E4F49534521ull)) + 2 * 0x9E3779B97F4A7C15ull;
    const uint32_t n = 1u << po2, act = layout_active_rows(po2, l->noise_rows);
    const std::vector<LayoutColumn> cols = l->columns(w_data);
    for (uint32_t c = 0; c < w_data; ++c) {
        const LayoutColumn& k = cols[c];
        uint32_t* out = data_out + (size_t)c * n;
        for (uint32_t r = 0; r < records; ++r) out[r] = layout_encode(((uint32_t)le(BX_SEGMENT_WIRE_BYTES + 4 * ((size_t)r * l->stride + k.word), 4) >> k.shift) & k.mask);
        for (uint32_t r = records; r < act; ++r) out[r] = k.pad;
        for (uint32_t r = act; r < n; ++r) out[r] = synth_word(nseed, c, r);
    }
    return nullptr;
} catch (...) {
    return "bx_trace_layout_data_host: out of host memory";
}

const char* bx_trace_layout_control_id_host_hashfn(const bx_trace_layout* l, uint32_t po2, const char* hashfn, uint32_t id_out[8]) try {
    using namespace bx;
    const int suite = suite_of(hashfn);
    if (suite < 0) return "bx_trace_layout_control_id_host: unknown hashfn (\"poseidon2\" or \"sha-256\")";
    if (!l || !id_out) return "bx_trace_layout_control_id_host: null argument";
    if (po2 < 9 || po2 > 24) return "bx_trace_layout_control_id_host: shape out of range (po2 in [9, 24])";
    if (const char* e = cached_id(l, po2, suite, id_out)) {
        if (e != g_err) snprintf(g_err, sizeof g_err, "%s", e);
        return g_err;
    }
    return nullptr;
} catch (...) {
    return "bx_trace_layout_control_id_host: out of host memory";
}

}  // extern "C"
