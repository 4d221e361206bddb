// trace_layout_check.cpp — the host half of trace layouts (include/bx_layout.h; csrc/trace_layout_host.cpp, control_id.cpp) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_trace_layout_cpu.py:
//   1. descriptor fuzzing: seeded descriptors, well-formed and malformed, through bx_trace_layout_create; each is compiled or refused as
//      the rules restated HERE say, every refusal by its message, in the header's order;
//   2. the host fills at po2 1, 3, 6 and 9 against a restatement of the header's text: every code kind, strides 1, 2, 3, 31, 32, 33 and
//      128, R in {0, 1, A-1, A}, noise_rows 0 and 1994, shift + bits = 32, bits 1 and 30, payload words all 0 and all 0xFFFFFFFF, both
//      payload refusals with the output still poison;
//   3. control IDs: a layout that restates the lookup circuit's code group gives bx_lookup_control_id_host_hashfn's ID at po2 9, w_code
//      4, under both suites; one that restates the synthetic circuit's gives bx_synthetic_control_id_host's.
// Nothing here includes a source of the library: only the public headers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "bx_layout.h"
#include "bx_lookup.h"

namespace {
constexpr uint32_t P = 2013265921u;
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr uint32_t POISON = 0xDEADBEEFu;
int g_failures = 0;

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
            if (++g_failures > 20) exit(1);   \
        }                                     \
    } while (0)

uint64_t mix64(uint64_t x) {
    uint64_t z = x + GOLDEN;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint32_t word(uint64_t s, uint32_t c, uint32_t r) {
    const uint32_t v = (uint32_t)(mix64(s ^ (((uint64_t)c << 32) | r)) >> 33);
    return v >= P ? v - P : v;
}
uint32_t holds(uint32_t x) { return (uint32_t)(((uint64_t)x << 32) % P); }  // the word of the value x

struct Rng {
    uint64_t s;
    uint64_t next() { return s = mix64(s); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
    bool chance(uint32_t one_in) { return below(one_in) == 0; }
};

struct Desc {
    std::vector<bx_layout_code_col> code;
    std::vector<uint32_t> table;
    std::vector<bx_layout_field> fields;
    uint32_t stride = 1, noise_rows = 1994, n_globals = 0;
    uint32_t n_code_override = UINT32_MAX;  // n_code as handed over, when it is not code.size()
    bx_trace_layout_desc c() const {
        return bx_trace_layout_desc{code.data(), n_code_override != UINT32_MAX ? n_code_override : (uint32_t)code.size(), table.data(), (uint32_t)table.size(),
                                    fields.data(), (uint32_t)fields.size(), stride, noise_rows, n_globals};
    }
};

// the rules of bx_trace_layout_create restated: "" = compiled, else what the refusal must contain.  Rule by rule over the whole
// description, in the header's order.
std::string expected(const Desc& d) {
    char m[256];
    const uint32_t n_code = d.n_code_override != UINT32_MAX ? d.n_code_override : (uint32_t)d.code.size();
    for (uint32_t c = 0; c < n_code; ++c)
        if (d.code[c].kind > 6) return snprintf(m, sizeof m, "code column %u: unknown kind %u", c, d.code[c].kind), m;
    for (uint32_t c = 0; c < n_code; ++c) {
        if (d.code[c].kind == BX_LAYOUT_CONST && d.code[c].a >= P) return snprintf(m, sizeof m, "code column %u: CONST value %u is not below P", c, d.code[c].a), m;
        if (d.code[c].kind == BX_LAYOUT_PERIODIC && d.code[c].a > 12) return snprintf(m, sizeof m, "code column %u: PERIODIC period 2^%u is above 2^12", c, d.code[c].a), m;
    }
    for (uint32_t c = 0; c < n_code; ++c)
        if (d.code[c].kind == BX_LAYOUT_PERIODIC && (uint64_t)d.code[c].b + (1ull << d.code[c].a) > d.table.size())
            return snprintf(m, sizeof m, "code column %u: PERIODIC window [%u, ", c, d.code[c].b), m;
    for (size_t i = 0; i < d.table.size(); ++i)
        if (d.table[i] >= P) return snprintf(m, sizeof m, "table value %zu (%u) is not below P", i, d.table[i]), m;
    if (d.stride < 1 || d.stride > 128) return snprintf(m, sizeof m, "stride %u is not in 1 .. 128", d.stride), m;
    const size_t nf = d.fields.size();
    for (size_t i = 0; i < nf; ++i)
        if (d.fields[i].word >= d.stride) return snprintf(m, sizeof m, "field %zu: word %u is not below the stride %u", i, d.fields[i].word, d.stride), m;
    for (size_t i = 0; i < nf; ++i)
        if (d.fields[i].bits < 1 || d.fields[i].bits > 30) return snprintf(m, sizeof m, "field %zu: bits %u is not in 1 .. 30", i, d.fields[i].bits), m;
    for (size_t i = 0; i < nf; ++i)
        if ((uint64_t)d.fields[i].shift + d.fields[i].bits > 32) return snprintf(m, sizeof m, "field %zu: shift %u + bits %u is above 32", i, d.fields[i].shift, d.fields[i].bits), m;
    for (size_t i = 0; i < nf; ++i)
        if (d.fields[i].pad >= (1u << d.fields[i].bits)) return snprintf(m, sizeof m, "field %zu: pad %u is not below 2^%u", i, d.fields[i].pad, d.fields[i].bits), m;
    for (size_t i = 0; i < nf; ++i)
        for (size_t j = 0; j < i; ++j)
            if (d.fields[j].col == d.fields[i].col)
                return snprintf(m, sizeof m, "field %zu: column %u is named a second time (first by field %zu)", i, d.fields[i].col, j), m;
    if (n_code == 0 || n_code >= 65536) return snprintf(m, sizeof m, "n_code %u is not in 1 .. 65535", n_code), m;
    for (size_t i = 0; i < nf; ++i)
        if (d.fields[i].col >= 65535) return snprintf(m, sizeof m, "field %zu: column %u is not below 65535", i, d.fields[i].col), m;
    if (d.n_globals > 64) return snprintf(m, sizeof m, "n_globals %u is above BX_MAX_GLOBALS = 64", d.n_globals), m;
    return "";
}

Desc well_formed(Rng& g) {
    Desc d;
    d.stride = 1 + g.below(128);
    d.noise_rows = g.chance(2) ? 1994 : g.below(3000);
    d.n_globals = g.below(65);
    d.table.resize(g.below(40));
    for (uint32_t& v : d.table) v = g.chance(8) ? P - 1 : g.below(P);
    d.code.resize(1 + g.below(12));
    for (bx_layout_code_col& k : d.code) {
        k.kind = g.below(7), k.a = (uint32_t)g.next(), k.b = (uint32_t)g.next();
        if (k.kind == BX_LAYOUT_CONST) k.a = g.below(P);
        if (k.kind == BX_LAYOUT_PERIODIC) {
            if (d.table.empty()) {
                k.kind = BX_LAYOUT_FIRST;
                continue;
            }
            k.a = 0;
            while (k.a < 12 && (2u << k.a) <= d.table.size() && g.chance(2)) ++k.a;
            k.b = g.below((uint32_t)d.table.size() - (1u << k.a) + 1);
        }
    }
    d.fields.resize(g.below(10));
    uint32_t col = g.below(3);
    for (bx_layout_field& f : d.fields) {
        f.col = col, col += 1 + g.below(3);
        f.word = g.below(d.stride);
        f.bits = 1 + g.below(30);
        f.shift = g.below(33 - f.bits);
        f.pad = g.below(1u << f.bits);
    }
    if (!d.fields.empty() && g.chance(6)) d.fields.back().col = 65534;
    return d;
}
// one defect of a random kind; several calls stack defects, and the FIRST broken rule in the header's order is the refusal
void damage(Desc& d, Rng& g) {
    bx_layout_code_col& k = d.code[g.below((uint32_t)d.code.size())];
    bx_layout_field* f = d.fields.empty() ? nullptr : &d.fields[g.below((uint32_t)d.fields.size())];
    switch (g.below(14)) {
    case 0: k.kind = 7 + g.below(5) * 1000; break;
    case 1: k.kind = BX_LAYOUT_CONST, k.a = P + g.below(100); break;
    case 2: k.kind = BX_LAYOUT_PERIODIC, k.a = 13 + g.below(40), k.b = 0; break;
    case 3: {  // a window that ends one to three values behind the table, or far behind it
        k.kind = BX_LAYOUT_PERIODIC, k.a = g.below(13);
        const uint32_t period = 1u << k.a, size = (uint32_t)d.table.size();
        k.b = g.chance(3) ? 0xFFFFFF00u : (size >= period ? size - period + 1 + g.below(3) : g.below(3));
        break;
    }
    case 4: if (!d.table.empty()) d.table[g.below((uint32_t)d.table.size())] = g.chance(2) ? P : 0xFFFFFFFFu; break;
    case 5: d.stride = g.chance(2) ? 0 : 129 + g.below(1000); break;
    case 6: if (f) f->word = d.stride + g.below(3); break;
    case 7: if (f) f->bits = g.chance(2) ? 0 : 31 + g.below(5); break;
    case 8: if (f) f->shift = 33 - f->bits + g.below(4); break;
    case 9: if (f && f->bits < 32) f->pad = (1u << f->bits) + g.below(4); break;
    case 10: if (f && d.fields.size() > 1) f->col = d.fields[g.below((uint32_t)d.fields.size())].col; break;
    case 11: d.n_code_override = 0; break;
    case 12: if (f) f->col = 65535 + g.below(3) * 70000; break;
    default: d.n_globals = 65 + g.below(1000); break;
    }
}

void fuzz_descriptors() {
    int compiled = 0, refused = 0;
    // what tells the refusals apart: rule 2 has two messages
    const char* rules[15] = {"unknown kind", "CONST value", "PERIODIC period", "PERIODIC window", "table value", "is not in 1 .. 128", "is not below the stride",
                             "is not in 1 .. 30", "is above 32", "is not below 2^", "second time", "is not in 1 .. 65535", "is not below 65535", "n_globals", nullptr};
    int by_rule[15] = {0};
    for (uint64_t seed = 1; seed <= 4000; ++seed) {
        Rng g{seed * 0x1234567ull};
        Desc d = well_formed(g);
        const uint32_t defects = seed % 3 == 0 ? 0 : 1 + g.below(3);
        for (uint32_t k = 0; k < defects; ++k) damage(d, g);
        const std::string want = expected(d);
        const bx_trace_layout_desc c = d.c();
        bx_trace_layout* l = (bx_trace_layout*)(uintptr_t)1;
        const char* msg = bx_trace_layout_create(&c, &l);
        if (want.empty()) {
            CHECK(msg == nullptr && l != nullptr && l != (bx_trace_layout*)(uintptr_t)1, "seed %llu: a well-formed descriptor was refused: %s", (unsigned long long)seed, msg ? msg : "(no layout)");
            if (!msg && l) {
                bx_trace_layout_info info;
                CHECK(bx_trace_layout_info_get(l, &info) == nullptr, "info_get");
                uint32_t top = 0;
                for (const bx_layout_field& f : d.fields) top = f.col + 1 > top ? f.col + 1 : top;
                CHECK(info.n_code == d.code.size() && info.n_table == d.table.size() && info.n_fields == d.fields.size() && info.stride == d.stride &&
                          info.noise_rows == d.noise_rows && info.n_globals == d.n_globals && info.min_w_data == top,
                      "seed %llu: info differs from the descriptor", (unsigned long long)seed);
                bx_trace_layout_destroy(l);
                ++compiled;
            }
        } else {
            CHECK(msg != nullptr && l == nullptr, "seed %llu: a malformed descriptor compiled (wanted: %s)", (unsigned long long)seed, want.c_str());
            if (msg) {
                CHECK(strncmp(msg, "trace_layout: ", 14) == 0 && strstr(msg, want.c_str()) != nullptr, "seed %llu: refused with \"%s\", wanted \"%s\"", (unsigned long long)seed, msg,
                      want.c_str());
                for (int r = 0; rules[r]; ++r)
                    if (strstr(msg, rules[r])) {
                        ++by_rule[r];
                        break;
                    }
                ++refused;
            } else if (l) {
                bx_trace_layout_destroy(l);
            }
        }
    }
    CHECK(compiled > 1000 && refused > 1500, "the fuzz is lopsided: %d compiled, %d refused", compiled, refused);
    for (int r = 0; rules[r]; ++r) CHECK(by_rule[r] >= 5, "\"%s\" was the refusal only %d times", rules[r], by_rule[r]);
    // null arguments come before every rule
    bx_trace_layout* l = nullptr;
    bx_trace_layout_desc bad{nullptr, 3, nullptr, 0, nullptr, 0, 0, 0, 99};
    CHECK(strstr(bx_trace_layout_create(&bad, &l), "null argument") != nullptr, "a null code array");
    CHECK(strstr(bx_trace_layout_create(nullptr, &l), "null argument") != nullptr, "a null descriptor");
    printf("descriptors: %d compiled, %d refused\n", compiled, refused);
}

// ---- the host fills against the header's text ----
uint32_t active_rows(uint32_t po2, uint32_t noise_rows) {
    const uint32_t n = 1u << po2;
    return n - (noise_rows < n / 4 ? noise_rows : n / 4);
}
uint32_t code_cell(const Desc& d, uint32_t c, uint32_t r, uint32_t po2) {
    const uint32_t n = 1u << po2, A = active_rows(po2, d.noise_rows), a = d.code[c].a, b = d.code[c].b;
    switch (d.code[c].kind) {
    case BX_LAYOUT_CONST: return holds(a);
    case BX_LAYOUT_FIRST: return r == 0 ? holds(1) : 0;
    case BX_LAYOUT_LAST: return r == A - 1 - a ? holds(1) : 0;
    case BX_LAYOUT_ACTIVE: return r < A - a ? holds(1) : 0;
    case BX_LAYOUT_ROW: {
        const uint32_t below = a ? a : n;
        return r < (below < n ? below : n) ? holds(r) : 0;
    }
    case BX_LAYOUT_PERIODIC: return holds(d.table[b + (r % (1u << a))]);
    default: return word((uint64_t)a | ((uint64_t)b << 32), c, r);
    }
}
std::vector<uint8_t> segment_of(uint32_t po2, uint64_t seed, const std::vector<uint32_t>& payload, size_t extra_bytes = 0) {
    std::vector<uint8_t> s(BX_SEGMENT_MAGIC, BX_SEGMENT_MAGIC + 8);  // "BXSYNSEG" | index u64 | po2 u32 | seed u64, little endian
    for (int k = 0; k < 8; ++k) s.push_back(k == 0 ? 7 : 0);
    for (int k = 0; k < 4; ++k) s.push_back((uint8_t)(po2 >> (8 * k)));
    for (int k = 0; k < 8; ++k) s.push_back((uint8_t)(seed >> (8 * k)));
    for (uint32_t w : payload)
        for (int k = 0; k < 4; ++k) s.push_back((uint8_t)(w >> (8 * k)));
    s.resize(s.size() + extra_bytes, 0xAB);
    return s;
}
bx_trace_layout* compile(const Desc& d) {
    const bx_trace_layout_desc c = d.c();
    bx_trace_layout* l = nullptr;
    const char* msg = bx_trace_layout_create(&c, &l);
    CHECK(msg == nullptr, "a layout of the fills was refused: %s", msg);
    if (msg) exit(1);
    return l;
}

void check_code_fill() {
    for (uint32_t noise : {0u, 1994u}) {
        Desc d;
        d.noise_rows = noise;
        d.table = {7, 1, 2, P - 1, 0};
        d.code = {{BX_LAYOUT_CONST, 0, 0}, {BX_LAYOUT_CONST, P - 1, 0}, {BX_LAYOUT_FIRST, 0, 0}, {BX_LAYOUT_LAST, 0, 0}, {BX_LAYOUT_LAST, 1, 0}, {BX_LAYOUT_ACTIVE, 0, 0},
                  {BX_LAYOUT_ACTIVE, 1, 0}, {BX_LAYOUT_ROW, 0, 0}, {BX_LAYOUT_ROW, 1, 0}, {BX_LAYOUT_ROW, 5, 0}, {BX_LAYOUT_ROW, 1000000, 0}, {BX_LAYOUT_PERIODIC, 0, 0},
                  {BX_LAYOUT_PERIODIC, 2, 1}, {BX_LAYOUT_WORD, 0x524F4C21u, 0x434F4E54u}, {BX_LAYOUT_WORD, 1, 0}};
        bx_trace_layout* l = compile(d);
        for (uint32_t po2 : {1u, 3u, 6u, 9u}) {
            const uint32_t n = 1u << po2;
            std::vector<uint32_t> got(d.code.size() * n, POISON);
            const char* msg = bx_trace_layout_code_host(l, po2, got.data());
            CHECK(msg == nullptr, "code_host at po2 %u: %s", po2, msg);
            for (uint32_t c = 0; c < d.code.size(); ++c)
                for (uint32_t r = 0; r < n; ++r)
                    CHECK(got[c * n + r] == code_cell(d, c, r, po2), "noise %u po2 %u: code cell (%u, %u) is %u, the text says %u", noise, po2, c, r, got[c * n + r],
                          code_cell(d, c, r, po2));
        }
        bx_trace_layout_destroy(l);
    }
    // LAST / ACTIVE with a >= A: refused where the shape is known, nothing written
    for (uint32_t kind : {(uint32_t)BX_LAYOUT_LAST, (uint32_t)BX_LAYOUT_ACTIVE}) {
        Desc d;
        d.code = {{BX_LAYOUT_FIRST, 0, 0}, {kind, 6, 0}};  // po2 3: A = 6
        bx_trace_layout* l = compile(d);
        std::vector<uint32_t> got(2 * 8, POISON);
        const char* msg = bx_trace_layout_code_host(l, 3, got.data());
        CHECK(msg && strstr(msg, "code column 1") && strstr(msg, "6 active rows"), "a = A was not refused: %s", msg ? msg : "(null)");
        for (uint32_t w : got) CHECK(w == POISON, "a refused code fill wrote");
        d.code[1].a = 5;
        bx_trace_layout* ok = compile(d);
        CHECK(bx_trace_layout_code_host(ok, 3, got.data()) == nullptr, "a = A - 1 was refused");
        bx_trace_layout_destroy(ok);
        bx_trace_layout_destroy(l);
    }
}

void check_data_fill() {
    long cells = 0;
    for (uint32_t stride : {1u, 2u, 3u, 31u, 32u, 33u, 128u})
        for (uint32_t noise : {0u, 1994u})
            for (uint32_t po2 : {1u, 3u, 6u, 9u}) {
                Rng g{stride * 1000003ull + noise * 31 + po2};
                Desc d;
                d.stride = stride, d.noise_rows = noise;
                d.code = {{BX_LAYOUT_FIRST, 0, 0}};
                // columns 0..5; column 3 has no field.  bits 1 and 30, shift + bits = 32, a word feeding two fields
                d.fields = {{0, stride - 1, 31, 1, 1}, {1, 0, 2, 30, (1u << 30) - 1}, {2, stride / 2, 0, 30, 0}, {4, stride - 1, 0, 17, 77}, {5, g.below(stride), 9, 23, 1u << 22}};
                const uint32_t w_data = 7;  // column 6: beyond every field
                bx_trace_layout* l = compile(d);
                const uint32_t n = 1u << po2, A = active_rows(po2, noise);
                for (uint32_t R : {0u, 1u, A - 1, A})
                    for (int fill = 0; fill < 3; ++fill) {
                        std::vector<uint32_t> payload((size_t)R * stride);
                        for (uint32_t& w : payload) w = fill == 0 ? (uint32_t)g.next() : (fill == 1 ? 0u : 0xFFFFFFFFu);
                        const uint64_t seed = g.next(), given = g.next();
                        const std::vector<uint8_t> seg = segment_of(po2, seed, payload);
                        for (int with_seed = 0; with_seed < 2; ++with_seed) {
                            std::vector<uint32_t> got((size_t)w_data * n, POISON);
                            const char* msg = bx_trace_layout_data_host(l, po2, seg.data(), seg.size(), with_seed ? &given : nullptr, got.data(), w_data);
                            CHECK(msg == nullptr, "data_host stride %u po2 %u R %u: %s", stride, po2, R, msg);
                            const uint64_t nseed = (with_seed ? given : mix64(seed ^ 0x5A4B4E4F49534521ull)) + 2 * GOLDEN;
                            for (uint32_t c = 0; c < w_data; ++c) {
                                const bx_layout_field* f = nullptr;
                                for (const bx_layout_field& q : d.fields)
                                    if (q.col == c) f = &q;
                                for (uint32_t r = 0; r < n; ++r, ++cells) {
                                    uint32_t want;
                                    if (r >= A) want = word(nseed, c, r);
                                    else if (!f) want = 0;
                                    else if (r < R) want = holds((payload[(size_t)r * stride + f->word] >> f->shift) & (uint32_t)((1ull << f->bits) - 1));
                                    else want = holds(f->pad);
                                    CHECK(got[(size_t)c * n + r] == want, "stride %u noise %u po2 %u R %u fill %d: data cell (%u, %u) is %u, the text says %u", stride, noise, po2,
                                          R, fill, c, r, got[(size_t)c * n + r], want);
                                }
                            }
                        }
                    }
                // the two payload refusals, each by its own message, the output still poison
                std::vector<uint32_t> got((size_t)w_data * n, POISON);
                const std::vector<uint8_t> ragged = segment_of(po2, 1, std::vector<uint32_t>(stride, 5u), stride == 1 ? 2 : 4);
                const char* msg = bx_trace_layout_data_host(l, po2, ragged.data(), ragged.size(), nullptr, got.data(), w_data);
                CHECK(msg && strstr(msg, "is not a whole number of"), "a ragged payload: %s", msg ? msg : "(accepted)");
                const std::vector<uint8_t> long_one = segment_of(po2, 1, std::vector<uint32_t>((size_t)(A + 1) * stride, 5u));
                msg = bx_trace_layout_data_host(l, po2, long_one.data(), long_one.size(), nullptr, got.data(), w_data);
                CHECK(msg && strstr(msg, "active rows"), "R = A + 1: %s", msg ? msg : "(accepted)");
                msg = bx_trace_layout_data_host(l, po2, long_one.data(), BX_SEGMENT_WIRE_BYTES, nullptr, got.data(), 5);
                CHECK(msg && strstr(msg, "a field names data column 5"), "w_data below a field's column: %s", msg ? msg : "(accepted)");
                for (uint32_t w : got) CHECK(w == POISON, "a refused data fill wrote");
                bx_trace_layout_destroy(l);
            }
    printf("host fills: %ld data cells\n", cells);
}

// ---- the base table's host entries ----
void check_table() {
    Desc d;
    d.noise_rows = 0, d.stride = 2, d.n_globals = 3;
    d.code = {{BX_LAYOUT_FIRST, 0, 0}, {BX_LAYOUT_LAST, 600, 0}};
    d.fields = {{4, 1, 0, 8, 0}};
    bx_trace_layout* l = compile(d);
    const bx_circuit_ops* ops = bx_trace_layout_ops(l);
    CHECK(ops && ops->normalize && ops->taps && ops->n_globals && ops->eval_check && ops->constraints_at && ops->check_code, "the table lacks a host entry");
    CHECK(!ops->create && !ops->code_group && !ops->witgen && !ops->accumulate, "this program has no device half: its entries are the library's to add");
    bx_segment_params s{10, 2, 5, 4, 0, 0};
    CHECK(ops->normalize(ops->user, &s) == nullptr && s.cons_terms == 0 && s.cons_degree == 0, "a fitting shape was refused or changed");
    CHECK(ops->n_globals(ops->user, &s) == 3, "n_globals");
    uint32_t backs[BX_MAX_TAPS];
    for (int g = 0; g < 3; ++g) CHECK(ops->taps(ops->user, &s, g, 1, backs) == 1 && backs[0] == 0, "taps is not {0}");
    const struct {
        bx_segment_params shape;
        const char* match;
    } bad[] = {{{10, 2, 5, 4, 1, 0}, "cons_terms and cons_degree"}, {{10, 2, 5, 4, 0, 2}, "cons_terms and cons_degree"}, {{10, 3, 5, 4, 0, 0}, "w_code is 3, the layout has 2"},
               {{10, 2, 4, 4, 0, 0}, "w_data is 4, a field names data column 4"}, {{9, 2, 5, 4, 0, 0}, "LAST with a = 600"}, {{0, 2, 5, 4, 0, 0}, "po2 must be"},
               {{25, 2, 5, 4, 0, 0}, "po2 must be"}};
    for (const auto& b : bad) {
        bx_segment_params shape = b.shape;
        const char* msg = ops->normalize(ops->user, &shape);
        CHECK(msg && strstr(msg, b.match), "normalize: wanted \"%s\", got \"%s\"", b.match, msg ? msg : "(accepted)");
    }
    uint32_t out[4];
    const char* msg = ops->constraints_at(ops->user, &s, nullptr, out, out, out, out);
    CHECK(msg && strstr(msg, "bx_cons_circuit_create"), "constraints_at of the layout's own table");
    msg = ops->eval_check(ops->user, nullptr, nullptr, bx_buf{nullptr, 0}, bx_buf{nullptr, 0}, bx_buf{nullptr, 0}, bx_buf{nullptr, 0}, out, out, out);
    CHECK(msg && strstr(msg, "bx_cons_circuit_create"), "eval_check of the layout's own table");
    bx_trace_layout_destroy(l);
}

// ---- control IDs against the two normative circuits ----
void check_control_ids() {
    const uint32_t po2 = 9, wc = 4;
    Desc lk;
    lk.noise_rows = 1994;
    lk.code = {{BX_LAYOUT_FIRST, 0, 0}, {BX_LAYOUT_LAST, 0, 0}, {BX_LAYOUT_ROW, 1u << 8, 0}, {BX_LAYOUT_WORD, 0x55502121u, 0x4C4F4F4Bu}};  // B = 2^min(15, po2 - 1); "LOOKUP!!"
    Desc sy = lk;
    sy.code = {{BX_LAYOUT_FIRST, 0, 0}, {BX_LAYOUT_LAST, 0, 0}, {BX_LAYOUT_WORD, 0x524F4C21u, 0x434F4E54u}, {BX_LAYOUT_WORD, 0x524F4C21u, 0x434F4E54u}};  // "CONTROL!"
    bx_trace_layout *l_lk = compile(lk), *l_sy = compile(sy);
    uint32_t got[8], want[8];
    for (const char* suite : {"poseidon2", "sha-256"}) {
        const char* msg = bx_trace_layout_control_id_host_hashfn(l_lk, po2, suite, got);
        CHECK(msg == nullptr, "the lookup layout's ID under %s: %s", suite, msg);
        CHECK(bx_lookup_control_id_host_hashfn(po2, wc, suite, want) == nullptr, "the lookup circuit's ID");
        CHECK(memcmp(got, want, 32) == 0, "the lookup layout's control ID under %s is not the lookup circuit's", suite);
        msg = bx_trace_layout_control_id_host_hashfn(l_sy, po2, suite, got);
        CHECK(msg == nullptr, "the synthetic layout's ID under %s: %s", suite, msg);
        CHECK(bx_synthetic_control_id_host_hashfn(po2, wc, suite, want) == nullptr, "the synthetic circuit's ID");
        CHECK(memcmp(got, want, 32) == 0, "the synthetic layout's control ID under %s is not the synthetic circuit's", suite);
    }
    CHECK(bx_synthetic_control_id_host(po2, wc, want) == nullptr && memcmp(got, want, 32) != 0, "the SHA-256 ID equals the Poseidon2 one");
    // check_code: the cached ID accepts its own root and refuses another; a second call is served from the cache
    const bx_circuit_ops* ops = bx_trace_layout_ops(l_sy);
    bx_segment_params shape{po2, wc, 1, 4, 0, 0};
    CHECK(ops->check_code(ops->user, &shape, want) == nullptr && ops->check_code(ops->user, &shape, want) == nullptr, "check_code refuses the layout's own control ID");
    want[3] ^= 1u;
    const char* msg = ops->check_code(ops->user, &shape, want);
    CHECK(msg && strstr(msg, "control ID"), "check_code accepts another root");
    // a different CONST column is a different circuit
    Desc other = sy;
    other.code[3] = {BX_LAYOUT_CONST, 5, 0};
    bx_trace_layout* l_other = compile(other);
    uint32_t id_other[8];
    CHECK(bx_trace_layout_control_id_host_hashfn(l_other, po2, "poseidon2", id_other) == nullptr, "the other layout's ID");
    CHECK(bx_trace_layout_control_id_host_hashfn(l_sy, po2, "poseidon2", got) == nullptr && memcmp(got, id_other, 32) != 0, "two code groups, one control ID");
    msg = bx_trace_layout_control_id_host_hashfn(l_sy, 8, "poseidon2", got);
    CHECK(msg && strstr(msg, "po2 in [9, 24]"), "po2 8");
    msg = bx_trace_layout_control_id_host_hashfn(l_sy, po2, "blake2b", got);
    CHECK(msg && strstr(msg, "unknown hashfn"), "an unknown suite");
    bx_trace_layout_destroy(l_other);
    bx_trace_layout_destroy(l_sy);
    bx_trace_layout_destroy(l_lk);
}
}  // namespace

// the library's table lives in circuit.hip next to the device stages; control_id.cpp names it only to tell the built-in circuits from
// plug-ins, which nothing here asks
extern "C" const bx_circuit_ops* bx_synthetic_circuit(void) { return nullptr; }

int main() {
    fuzz_descriptors();
    check_code_fill();
    check_data_fill();
    check_table();
    check_control_ids();
    if (g_failures) {
        printf("trace_layout_check: %d failures\n", g_failures);
        return 1;
    }
    printf("trace_layout_check ok\n");
    return 0;
}
