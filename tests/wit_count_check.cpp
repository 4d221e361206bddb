// wit_count_check.cpp — stand-alone checker of a witness program's multiplicity columns on the host (bx_wit_program_create_counted and
// bx_wit_program_run_host in csrc/program_compile.cpp and csrc/cons_program_host.cpp; include/bx_program.h, "multiplicity columns", is the text), built with
// -fsanitize=address,undefined by tests/test_wit_count_cpu.py and run as a process of its own.
//
// 3 000 seeded descriptors with count lists, well-formed and malformed, go through create: every one is either refused (with a message)
// or compiled, and a compiled one must keep every rule of the text, which is restated below and shares nothing with the library but
// the field arithmetic of fp.hpp.  Every compiled program is run by bx_wit_program_run_host at po2 1, 3 and 6 over random, all-0,
// all-(P - 1) and alternating columns and compared with a DIRECT evaluation: the step list row by row, then every count by a plain
// tally.  The count columns are poisoned first, so a row at or above `rows` that was written shows.  A count that does not fit the
// shape (rows > N, bins > N with rows == 0, a column beyond the width) must be refused by message with nothing written.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
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

constexpr uint32_t W_CODE = 2, W_DATA = 10;
constexpr uint32_t POISON = P - 1;

struct Count {
    uint32_t col, bins, rows, n_sources;  // n_sources may lie (malformed cases); `sources` always holds at least that many
    std::vector<uint32_t> sources;
};
struct Case {
    std::vector<bx_cons_step> steps;
    std::vector<bx_cons_tap> taps;
    std::vector<Count> counts;
};

// Well-formed: data columns 0..3 are free, 4 and 5 may be SET (each a small expression of free cells and of the other SET column),
// 6..9 may be count columns; the sources of a count are distinct columns of 0..5.
static Case well_formed() {
    Case c;
    const auto tap = [&](uint32_t g, uint32_t col, uint32_t back) {
        c.taps.push_back(bx_cons_tap{g, col, back});
        return (uint32_t)c.taps.size() - 1;
    };
    uint32_t n_fp = 0;
    const auto leaf = [&]() {
        const uint32_t k = below(4);
        if (k == 0) c.steps.push_back(bx_cons_step{BX_CONS_CONST, below(P), 0, 0, 0});
        else if (k == 1) c.steps.push_back(bx_cons_step{BX_CONS_GET, tap(0, below(W_CODE), below(4)), 0, 0, 0});
        else c.steps.push_back(bx_cons_step{BX_CONS_GET, tap(1, below(4), below(4)), 0, 0, 0});
        return n_fp++;
    };
    for (uint32_t col = 4; col < 6; ++col) {
        if (below(3) == 0) continue;
        uint32_t v = leaf();
        for (uint32_t k = below(4); k; --k) {
            const uint32_t w = (col == 5 && below(2) && !c.steps.empty() && c.steps.back().op != BX_CONS_SET) ? v : leaf();
            const uint32_t r = below(3);
            c.steps.push_back(bx_cons_step{r == 0 ? BX_CONS_ADD : (r == 1 ? BX_CONS_SUB : BX_CONS_MUL), v, w, 0, 0});
            v = n_fp++;
        }
        c.steps.push_back(bx_cons_step{BX_CONS_SET, col, v, 0, 0});
    }
    static const uint32_t kRows[] = {0, 0, 1, 2, 3, 5, 8, 37, 64};
    uint32_t next_col = 6;
    for (uint32_t k = below(4); k && next_col < W_DATA; --k) {
        Count ct;
        ct.col = next_col;
        next_col += 1 + below(2);
        ct.rows = kRows[below(sizeof kRows / sizeof kRows[0])];
        const uint32_t limit = ct.rows ? ct.rows : (below(2) ? 2u : 64u);  // rows == 0: bins must fit the smallest N it will see, or be refused there
        ct.bins = 1 + below(limit);
        std::set<uint32_t> src;
        for (uint32_t q = 1 + below(6); q; --q) src.insert(below(6));
        ct.sources.assign(src.begin(), src.end());
        if (below(2)) std::swap(ct.sources.front(), ct.sources.back());  // not sorted
        ct.n_sources = (uint32_t)ct.sources.size();
        c.counts.push_back(ct);
    }
    return c;
}

static Case malformed() {
    Case c = well_formed();
    if (c.counts.empty()) c.counts.push_back(Count{6, 1, 0, 1, {0}});
    for (uint32_t hits = 1 + below(2); hits; --hits) {
        Count& ct = c.counts[below((uint32_t)c.counts.size())];
        switch (below(13)) {
        case 0: ct.col = (uint32_t)rnd() >> below(32); break;
        case 1: ct.col = 4 + below(2); break;                                       // perhaps a SET column
        case 2: ct.col = below(4); break;                                           // perhaps tapped, perhaps a source
        case 3: ct.sources.push_back(ct.sources[below((uint32_t)ct.sources.size())]), ct.n_sources++; break;  // a source twice
        case 4: ct.n_sources = 0; break;
        case 5: ct.sources.resize(65 + below(10), 1), ct.n_sources = (uint32_t)ct.sources.size(); break;
        case 6: ct.bins = 0; break;
        case 7: ct.bins = ct.rows + 1 + below(3); break;                            // above rows (valid when rows == 0)
        case 8: ct.bins = (1u << 24) + below(2); ct.rows = below(2) ? 0 : ct.bins; break;
        case 9: ct.sources[below((uint32_t)ct.sources.size())] = (uint32_t)rnd() >> below(32); break;
        case 10: ct.sources[0] = c.counts[below((uint32_t)c.counts.size())].col; break;  // a count column as a source
        case 11: c.counts.push_back(c.counts[below((uint32_t)c.counts.size())]); break;  // a column named by two counts
        default:
            while (c.counts.size() <= 16 + below(3)) c.counts.push_back(Count{(uint32_t)(100 + c.counts.size()), 1, 0, 1, {0}});
            break;
        }
    }
    return c;
}

// the rules of the text, restated: throws when create let a count list through that breaks one
static void check_rules(const Case& c, const std::map<uint32_t, size_t>& set_at) {
    if (c.counts.size() > 16) throw std::runtime_error("more than 16 counts");
    std::set<uint32_t> cols, all_sources, tapped;
    for (const bx_cons_step& s : c.steps)
        if (s.op == BX_CONS_GET && c.taps.at(s.a).group == 1) tapped.insert(c.taps[s.a].col);
    for (const Count& ct : c.counts) {
        if (ct.col > BX_CONS_MAX_COL) throw std::runtime_error("a count column above BX_CONS_MAX_COL");
        if (ct.n_sources < 1 || ct.n_sources > 64) throw std::runtime_error("no sources, or more than 64");
        if (ct.bins == 0 || ct.bins > (1u << 24) || (ct.rows && ct.bins > ct.rows)) throw std::runtime_error("bins out of range");
        if (ct.rows > (1u << 24)) throw std::runtime_error("rows above 2^24, the largest trace");
        if (!cols.insert(ct.col).second) throw std::runtime_error("a column named by two counts");
        if (set_at.count(ct.col)) throw std::runtime_error("a count column that is also SET");
        if (tapped.count(ct.col)) throw std::runtime_error("a count column read by a GET");
        std::set<uint32_t> mine;
        for (uint32_t q = 0; q < ct.n_sources; ++q) {
            if (ct.sources[q] > BX_CONS_MAX_COL) throw std::runtime_error("a source above BX_CONS_MAX_COL");
            if (!mine.insert(ct.sources[q]).second) throw std::runtime_error("a source named twice within one count");
            all_sources.insert(ct.sources[q]);
        }
    }
    for (uint32_t col : cols)
        if (all_sources.count(col)) throw std::runtime_error("a count column that is a source");
}

// the header's step table for one row (tests/wit_program_check.cpp checks the per-row compiler at length; here it feeds the counts)
static void direct_row(const Case& c, uint32_t po2, uint32_t r, const std::vector<uint32_t>& code, std::vector<uint32_t>& data) {
    const uint32_t n = 1u << po2;
    std::vector<uint32_t> fp;
    for (const bx_cons_step& s : c.steps) switch (s.op) {
        case BX_CONS_CONST: fp.push_back(fp_encode(s.a)); break;
        case BX_CONS_GET: {
            const bx_cons_tap& t = c.taps.at(s.a);
            fp.push_back((t.group == 0 ? code : data).at((size_t)t.col * n + ((r - t.back) & (n - 1u))));
            break;
        }
        case BX_CONS_ADD: fp.push_back(fp_add(fp.at(s.a), fp.at(s.b))); break;
        case BX_CONS_SUB: fp.push_back(fp_sub(fp.at(s.a), fp.at(s.b))); break;
        case BX_CONS_MUL: fp.push_back(fp_mul(fp.at(s.a), fp.at(s.b))); break;
        case BX_CONS_SET: data.at((size_t)s.a * n + r) = fp.at(s.b); break;
        default: throw std::runtime_error("an op that does not belong in a witness program");
        }
}
// "let c(v) be the number of pairs (source column s, row j < rows) whose cell, decoded, is the integer v"
static void direct_count(const Count& ct, uint32_t po2, std::vector<uint32_t>& data) {
    const uint32_t n = 1u << po2, rows = ct.rows ? ct.rows : n;
    std::map<uint32_t, uint32_t> tally;
    for (uint32_t q = 0; q < ct.n_sources; ++q)
        for (uint32_t j = 0; j < rows; ++j) ++tally[fp_decode(data.at((size_t)ct.sources[q] * n + j))];
    for (uint32_t r = 0; r < rows; ++r) data.at((size_t)ct.col * n + r) = r < ct.bins && tally.count(r) ? fp_encode(tally[r]) : 0u;
}

// random (small values, so that bins are hit), all 0, all P - 1, alternating 0 / P - 1
static void fill(std::vector<uint32_t>& v, uint32_t kind, uint32_t spread) {
    for (size_t i = 0; i < v.size(); ++i)
        v[i] = kind == 0 ? (below(4) ? fp_encode(below(spread)) : below(P)) : (kind == 1 ? 0u : (kind == 2 ? P - 1 : (i & 1 ? P - 1 : 0u)));
}

int main() {
    long compiled = 0, refused = 0, compiled_malformed = 0, ran = 0, shape_refused = 0, counted = 0, nonzero_bins = 0;
    for (uint32_t seed = 0; seed < 3000; ++seed) {
        g_state = 0xC0117ull * (seed + 1);
        const bool bad = seed % 3 == 2;
        const Case c = bad ? malformed() : well_formed();
        std::vector<bx_wit_count> counts;
        for (const Count& ct : c.counts) counts.push_back(bx_wit_count{ct.col, ct.bins, ct.rows, ct.n_sources, ct.sources.data()});
        bx_wit_program_desc d{c.steps.data(), c.steps.size(), c.taps.data(), c.taps.size(), nullptr, 0};
        bx_wit_program* prog = nullptr;
        const char* msg = bx_wit_program_create_counted(&d, counts.data(), counts.size(), &prog);
        if (msg) {
            if (prog || !*msg) {
                printf("seed %u: a refusal left a program behind or has no message\n", seed);
                return 1;
            }
            if (!bad) {
                printf("seed %u: a well-formed descriptor was refused: %s\n", seed, msg);
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
        std::map<uint32_t, size_t> set_at;
        for (size_t i = 0; i < c.steps.size(); ++i)
            if (c.steps[i].op == BX_CONS_SET) set_at.emplace(c.steps[i].a, i);
        try {
            check_rules(c, set_at);
        } catch (const std::exception& ex) {
            printf("seed %u: create accepted %s\n", seed, ex.what());
            return 1;
        }
        // what create kept is what it was given
        if (bx_wit_program_counts(prog) != c.counts.size()) {
            printf("seed %u: %u counts kept of %zu\n", seed, bx_wit_program_counts(prog), c.counts.size());
            return 1;
        }
        for (uint32_t k = 0; k < c.counts.size(); ++k) {
            uint32_t col = 0, bins = 0, rows = 0, ns = 0, src[64];
            const char* e = bx_wit_program_count_get(prog, k, &col, &bins, &rows, src, 64, &ns);
            const Count& ct = c.counts[k];
            if (e || col != ct.col || bins != ct.bins || rows != ct.rows || ns != ct.n_sources || memcmp(src, ct.sources.data(), 4 * ns) ||
                bx_wit_program_derives(prog, ct.col) != 1) {
                printf("seed %u: count %u is not what was given (%s)\n", seed, k, e ? e : "fields differ");
                return 1;
            }
        }
        uint32_t dummy[4];
        if (!bx_wit_program_count_get(prog, (uint32_t)c.counts.size(), dummy, dummy + 1, dummy + 2, nullptr, 0, dummy + 3)) {
            printf("seed %u: count_get past the end was not refused\n", seed);
            return 1;
        }
        std::set<uint32_t> count_cols;
        for (const Count& ct : c.counts) count_cols.insert(ct.col);
        for (uint32_t col = 0; col < 4; ++col)
            if (!count_cols.count(col) && bx_wit_program_derives(prog, col)) {
                printf("seed %u: derives(%u) is 1 for a free column\n", seed, col);
                return 1;
            }
        for (uint32_t po2 : {1u, 3u, 6u})
            for (uint32_t kind = 0; kind < 4; ++kind) {
                const uint32_t n = 1u << po2;
                bool fits = true;
                for (const Count& ct : c.counts) {
                    fits &= ct.rows <= n && (ct.rows || ct.bins <= n) && ct.col < W_DATA;
                    for (uint32_t q = 0; q < ct.n_sources; ++q) fits &= ct.sources[q] < W_DATA;
                }
                std::vector<uint32_t> code(W_CODE * (size_t)n), data(W_DATA * (size_t)n);
                fill(code, kind, n);
                fill(data, kind, 1 + below(2 * n));
                for (uint32_t col = 0; col < W_DATA; ++col)  // SET and count columns: poisoned
                    for (uint32_t r = 0; r < n && (col >= 4 || count_cols.count(col)); ++r) data[(size_t)col * n + r] = POISON;
                std::vector<uint32_t> got = data, want = data;
                const char* e = bx_wit_program_run_host(prog, po2, code.data(), W_CODE, got.data(), W_DATA);
                if (!fits) {
                    if (!e || !*e || got != data) {
                        printf("seed %u po2 %u: run_host took a count that does not fit the shape, or wrote before it refused\n", seed, po2);
                        return 1;
                    }
                    ++shape_refused;
                    continue;
                }
                if (e) {
                    printf("seed %u po2 %u: run_host: %s\n", seed, po2, e);
                    return 1;
                }
                for (uint32_t r = 0; r < n; ++r) direct_row(c, po2, n - 1 - r, code, want);  // rows in another order than the library's
                for (const Count& ct : c.counts) direct_count(ct, po2, want);
                if (got != want) {
                    size_t k = 0;
                    while (got[k] == want[k]) ++k;
                    printf("seed %u po2 %u pattern %u: data[%zu][%zu] is %u by run_host, %u by the definition\n", seed, po2, kind, k / n, k % n, got[k], want[k]);
                    return 1;
                }
                for (const Count& ct : c.counts) {
                    const uint32_t rows = ct.rows ? ct.rows : n;
                    for (uint32_t r = rows; r < n; ++r)
                        if (got[(size_t)ct.col * n + r] != POISON) {
                            printf("seed %u po2 %u: row %u of count column %u is at or above rows = %u and was written\n", seed, po2, r, ct.col, rows);
                            return 1;
                        }
                    for (uint32_t r = 0; r < rows; ++r) nonzero_bins += got[(size_t)ct.col * n + r] != 0;
                    ++counted;
                }
                ++ran;
            }
        bx_wit_program_destroy(prog);
    }
    printf("compiled %ld (of them malformed-but-valid %ld), refused %ld, runs %ld, refused for the shape %ld, counts evaluated %ld, non-zero multiplicities %ld\n",
           compiled, compiled_malformed, refused, ran, shape_refused, counted, nonzero_bins);
    if (compiled < 1500 || refused < 500 || ran < 5000 || shape_refused < 1000 || counted < 5000 || nonzero_bins < 5000) {
        printf("the case mix is too thin to mean anything\n");
        return 1;
    }
    printf("wit_count_check ok\n");
    return 0;
}
