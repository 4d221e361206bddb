// wit_sort_check.cpp — stand-alone checker of a witness program's sorted columns on the host (bx_wit_program_create_sorted and
// bx_wit_program_run_host in csrc/program_compile.cpp and csrc/cons_program_host.cpp; include/bx_program.h, "sorted columns", is the
// text), built with -fsanitize=address,undefined by tests/test_wit_sort_cpu.py and run as a process of its own.
//
// 3 000 seeded descriptors with sort lists, well-formed and malformed, some with a count, go through create: every one is either
// refused (with a message) or compiled, and a compiled one must keep every rule of the text, which is restated below and shares
// nothing with the library but the field arithmetic of fp.hpp.  Every compiled program is run by bx_wit_program_run_host at po2 1, 3
// and 6 over random, all-0, all-(P - 1), ascending, descending and few-distinct-values columns and compared with a DIRECT evaluation:
// the step list row by row, every sort by std::sort on (masked key tuple, row) — the row as an explicit last key, not a stable sort
// — and every count by a plain tally.  Dests and count columns are poisoned first, so a row at or above `rows` that was written
// shows, and every other column must still be as planted.  A sort that does not fit the shape (rows > N, a column beyond the width)
// must be refused by message with nothing written.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
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

constexpr uint32_t W_CODE = 2, W_DATA = 14;
constexpr uint32_t POISON = P - 1;
constexpr uint32_t COUNT_COL = 12;

struct Sort {
    uint32_t rows, n_keys, n_cols;  // n_keys and n_cols may lie (malformed cases); the vectors always hold at least that many
    std::vector<uint32_t> bits, sources, dests;
};
struct Count {
    uint32_t col, bins, rows;
    std::vector<uint32_t> sources;
};
struct Case {
    std::vector<bx_cons_step> steps;
    std::vector<bx_cons_tap> taps;
    std::vector<Sort> sorts;
    std::vector<Count> counts;
};

// Well-formed: data columns 0..3 are free, 4 and 5 may be SET, 6..11 and 13 may be dests, 12 may be a count column; the sources of a sort
// are distinct columns of 0..5, the sources of the count columns of 0..5 or a dest.
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
        for (uint32_t k = below(3); k; --k) {
            const uint32_t w = leaf(), r = below(3);
            c.steps.push_back(bx_cons_step{r == 0 ? BX_CONS_ADD : (r == 1 ? BX_CONS_SUB : BX_CONS_MUL), v, w, 0, 0});
            v = n_fp++;
        }
        c.steps.push_back(bx_cons_step{BX_CONS_SET, col, v, 0, 0});
    }
    static const uint32_t kRows[] = {0, 0, 1, 2, 3, 5, 8, 37, 64};
    static const uint32_t kBits[] = {1, 2, 3, 8, 9, 13, 16, 24, 31};
    uint32_t next_dest = 6;
    bool used_13 = false;
    for (uint32_t k = 1 + below(2); k; --k) {
        Sort s;
        s.rows = kRows[below(sizeof kRows / sizeof kRows[0])];
        const uint32_t room = 12 - next_dest;
        if (room == 0) break;
        s.n_cols = 1 + below(std::min(room, 4u));
        std::set<uint32_t> src;
        while (src.size() < s.n_cols) src.insert(below(6));
        s.sources.assign(src.begin(), src.end());
        if (below(2)) std::swap(s.sources.front(), s.sources.back());  // not sorted
        s.n_keys = 1 + below(s.n_cols);
        uint32_t total = 0;
        for (uint32_t q = 0; q < s.n_keys; ++q) {
            uint32_t b = kBits[below(sizeof kBits / sizeof kBits[0])];
            if (total + b > 64 - (s.n_keys - 1 - q)) b = 1;  // leave a bit for every key still to come
            s.bits.push_back(b);
            total += b;
        }
        for (uint32_t q = 0; q < s.n_cols; ++q) s.dests.push_back(next_dest++);
        if (below(4) == 0 && !used_13) s.dests.back() = 13, --next_dest, used_13 = true;
        c.sorts.push_back(s);
    }
    if (below(3) == 0) {  // a count over free columns and perhaps a dest
        Count ct;
        ct.col = COUNT_COL;
        ct.rows = kRows[below(sizeof kRows / sizeof kRows[0])];
        ct.bins = 1 + below(ct.rows ? ct.rows : 2u);
        ct.sources.push_back(below(4));
        if (below(2)) ct.sources.push_back(c.sorts[0].dests[0]);
        c.counts.push_back(ct);
    }
    return c;
}

static Case malformed() {
    Case c = well_formed();
    for (uint32_t hits = 1 + below(2); hits; --hits) {
        Sort& s = c.sorts[below((uint32_t)c.sorts.size())];
        switch (below(17)) {
        case 0: s.dests[below(s.n_cols)] = (uint32_t)rnd() >> below(32); break;
        case 1: s.dests[below(s.n_cols)] = 4 + below(2); break;  // perhaps a SET column
        case 2: s.dests[below(s.n_cols)] = below(4); break;      // perhaps tapped, perhaps a source
        case 3: s.sources.push_back(s.sources[below(s.n_cols)]), s.dests.push_back(13), s.n_cols++; break;  // a source twice (perhaps dest 13 twice)
        case 4: s.n_cols = 0; break;
        case 5:
            s.n_cols = 17 + below(4);
            s.sources.resize(s.n_cols, 1), s.dests.resize(s.n_cols, 7);
            break;
        case 6: s.n_keys = 0; break;
        case 7: s.n_keys = below(2) ? 5 : s.n_cols + 1, s.bits.resize(8, 1); break;  // valid when n_cols + 1 <= min(n_cols, 4): never
        case 8: s.bits[below(s.n_keys)] = below(2) ? 0 : 32 + below(40); break;
        case 9: std::fill(s.bits.begin(), s.bits.end(), 31u - below(2)); break;  // above 64 bits with three keys or more
        case 10: s.rows = (1u << 24) + below(2); break;                          // 2^24 itself is fine here, and fits no shape below
        case 11: s.dests[below(s.n_cols)] = COUNT_COL; break;                    // a count column when there is a count
        case 12: s.sources[below(s.n_cols)] = COUNT_COL; break;
        case 13: s.dests[below(s.n_cols)] = c.sorts[below((uint32_t)c.sorts.size())].dests[0]; break;  // a dest twice, unless it is itself
        case 14:
            while (c.sorts.size() <= 8 + below(3)) c.sorts.push_back(Sort{0, 1, 1, {8}, {0}, {(uint32_t)(100 + c.sorts.size())}});
            hits = 1;  // `s` is gone
            break;
        case 15: s.sources[below(s.n_cols)] = (uint32_t)rnd() >> below(32); break;
        default: s.dests[below(s.n_cols)] = 13 + below(60000); break;  // within BX_CONS_MAX_COL, beyond the width
        }
    }
    return c;
}

// the rules of the text, restated: throws when create let a sort list through that breaks one
static void check_rules(const Case& c, const std::map<uint32_t, size_t>& set_at) {
    if (c.sorts.size() > 8) throw std::runtime_error("more than 8 sorts");
    std::set<uint32_t> dests, all_sources, tapped, count_cols;
    for (const bx_cons_step& s : c.steps)
        if (s.op == BX_CONS_GET && c.taps.at(s.a).group == 1) tapped.insert(c.taps[s.a].col);
    for (const Count& ct : c.counts) count_cols.insert(ct.col);
    for (const Sort& s : c.sorts) {
        if (s.n_cols < 1 || s.n_cols > 16) throw std::runtime_error("no sources, or more than 16");
        if (s.n_keys < 1 || s.n_keys > 4 || s.n_keys > s.n_cols) throw std::runtime_error("n_keys out of range");
        if (s.rows > (1u << 24)) throw std::runtime_error("rows above 2^24");
        uint32_t total = 0;
        for (uint32_t q = 0; q < s.n_keys; ++q) {
            if (s.bits[q] < 1 || s.bits[q] > 31) throw std::runtime_error("a bits value of 0 or above 31");
            total += s.bits[q];
        }
        if (total > 64) throw std::runtime_error("more than 64 key bits");
        std::set<uint32_t> mine;
        for (uint32_t q = 0; q < s.n_cols; ++q) {
            if (s.sources[q] > BX_CONS_MAX_COL || s.dests[q] > BX_CONS_MAX_COL) throw std::runtime_error("a column above BX_CONS_MAX_COL");
            if (!mine.insert(s.sources[q]).second) throw std::runtime_error("a source named twice within one sort");
            if (count_cols.count(s.sources[q])) throw std::runtime_error("a source that is a count column");
            all_sources.insert(s.sources[q]);
            if (!dests.insert(s.dests[q]).second) throw std::runtime_error("a dest named twice");
            if (set_at.count(s.dests[q])) throw std::runtime_error("a dest that is SET");
            if (tapped.count(s.dests[q])) throw std::runtime_error("a dest named by a GET");
            if (count_cols.count(s.dests[q])) throw std::runtime_error("a dest that is a count column");
        }
    }
    for (uint32_t col : dests)
        if (all_sources.count(col)) throw std::runtime_error("a dest that is a source of a sort");
}

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
// "pi is the stable sort of rows [0, rows) by the key tuple, lexicographic, ties by ascending row": the row as the last key of a plain sort
static void direct_sort(const Sort& s, uint32_t po2, std::vector<uint32_t>& data) {
    const uint32_t n = 1u << po2, rows = s.rows ? s.rows : n;
    std::vector<std::array<uint32_t, 5>> order(rows);
    for (uint32_t r = 0; r < rows; ++r) {
        order[r].fill(0);
        for (uint32_t q = 0; q < s.n_keys; ++q) order[r][q] = fp_decode(data.at((size_t)s.sources[q] * n + r)) % (uint32_t)((uint64_t)1 << s.bits[q]);
        order[r][4] = r;
    }
    std::sort(order.begin(), order.end());
    std::vector<uint32_t> snapshot = data;
    for (uint32_t q = 0; q < s.n_cols; ++q)
        for (uint32_t r = 0; r < rows; ++r) data.at((size_t)s.dests[q] * n + r) = snapshot.at((size_t)s.sources[q] * n + order[r][4]);
}
static void direct_count(const Count& ct, uint32_t po2, std::vector<uint32_t>& data) {
    const uint32_t n = 1u << po2, rows = ct.rows ? ct.rows : n;
    std::map<uint32_t, uint32_t> tally;
    for (uint32_t src : ct.sources)
        for (uint32_t j = 0; j < rows; ++j) ++tally[fp_decode(data.at((size_t)src * n + j))];
    for (uint32_t r = 0; r < rows; ++r) data.at((size_t)ct.col * n + r) = r < ct.bins && tally.count(r) ? fp_encode(tally[r]) : 0u;
}

// random, all 0, all P - 1, ascending, descending, few distinct values
static void fill(std::vector<uint32_t>& v, uint32_t kind, uint32_t n) {
    for (size_t i = 0; i < v.size(); ++i) {
        const uint32_t r = (uint32_t)(i % n);
        v[i] = kind == 0 ? below(P) : kind == 1 ? 0u : kind == 2 ? P - 1 : kind == 3 ? fp_encode(r) : kind == 4 ? fp_encode(n - 1 - r) : fp_encode(below(3) * 1000003u);
    }
}

int main() {
    long compiled = 0, refused = 0, compiled_malformed = 0, ran = 0, shape_refused = 0, sorted = 0, moved = 0;
    for (uint32_t seed = 0; seed < 3000; ++seed) {
        g_state = 0x50A7ull * (seed + 1);
        const bool bad = seed % 3 == 2;
        const Case c = bad ? malformed() : well_formed();
        std::vector<bx_wit_sort> sorts;
        for (const Sort& s : c.sorts) sorts.push_back(bx_wit_sort{s.rows, s.n_keys, s.n_cols, s.bits.data(), s.sources.data(), s.dests.data()});
        std::vector<bx_wit_count> counts;
        for (const Count& ct : c.counts) counts.push_back(bx_wit_count{ct.col, ct.bins, ct.rows, (uint32_t)ct.sources.size(), ct.sources.data()});
        bx_wit_program_desc d{c.steps.data(), c.steps.size(), c.taps.data(), c.taps.size(), nullptr, 0};
        bx_wit_program* prog = nullptr;
        const char* msg = bx_wit_program_create_sorted(&d, counts.data(), counts.size(), sorts.data(), sorts.size(), &prog);
        if (msg) {
            if (prog || !*msg) {
                printf("seed %u: a refusal left a program behind or has no message\n", seed);
                return 1;
            }
            if (!bad) {
                printf("seed %u: a well-formed descriptor was refused: %s\n", seed, msg);
                return 1;
            }
            if (!strstr(msg, "sort")) {
                printf("seed %u: a refusal that does not name the sort list: %s\n", seed, msg);
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
        if (bx_wit_program_sorts(prog) != c.sorts.size() || bx_wit_program_counts(prog) != c.counts.size()) {
            printf("seed %u: %u sorts kept of %zu\n", seed, bx_wit_program_sorts(prog), c.sorts.size());
            return 1;
        }
        std::set<uint32_t> written;
        for (uint32_t k = 0; k < c.sorts.size(); ++k) {
            uint32_t rows = 0, nk = 0, nc = 0, bits[4] = {0, 0, 0, 0}, src[16], dst[16];
            const char* e = bx_wit_program_sort_get(prog, k, &rows, &nk, bits, src, dst, 16, &nc);
            const Sort& s = c.sorts[k];
            if (e || rows != s.rows || nk != s.n_keys || nc != s.n_cols || memcmp(bits, s.bits.data(), 4 * nk) || memcmp(src, s.sources.data(), 4 * nc) ||
                memcmp(dst, s.dests.data(), 4 * nc)) {
                printf("seed %u: sort %u is not what was given (%s)\n", seed, k, e ? e : "fields differ");
                return 1;
            }
            for (uint32_t q = 0; q < nc; ++q) {
                written.insert(dst[q]);
                if (bx_wit_program_derives(prog, dst[q]) != 1) {
                    printf("seed %u: derives(%u) is 0 for a dest\n", seed, dst[q]);
                    return 1;
                }
            }
        }
        uint32_t dummy[8];
        if (!bx_wit_program_sort_get(prog, (uint32_t)c.sorts.size(), dummy, dummy + 1, dummy + 2, nullptr, nullptr, 0, dummy + 6)) {
            printf("seed %u: sort_get past the end was not refused\n", seed);
            return 1;
        }
        for (const Count& ct : c.counts) written.insert(ct.col);
        for (uint32_t col = 0; col < 4; ++col)
            if (!written.count(col) && bx_wit_program_derives(prog, col)) {
                printf("seed %u: derives(%u) is 1 for a free column\n", seed, col);
                return 1;
            }
        for (uint32_t po2 : {1u, 3u, 6u})
            for (uint32_t kind = 0; kind < 6; ++kind) {
                const uint32_t n = 1u << po2;
                bool fits = true;
                for (const Sort& s : c.sorts) {
                    fits &= s.rows <= n;
                    for (uint32_t q = 0; q < s.n_cols; ++q) fits &= s.sources[q] < W_DATA && s.dests[q] < W_DATA;
                }
                for (const Count& ct : c.counts) fits &= ct.rows <= n && (ct.rows || ct.bins <= n);
                std::vector<uint32_t> code(W_CODE * (size_t)n), data(W_DATA * (size_t)n);
                fill(code, 0, n);
                fill(data, kind, n);
                for (uint32_t col = 0; col < W_DATA; ++col)  // SET columns, dests and count columns: poisoned
                    for (uint32_t r = 0; r < n && ((col >= 4 && col < 6) || written.count(col)); ++r) data[(size_t)col * n + r] = POISON;
                std::vector<uint32_t> got = data, want = data;
                const char* e = bx_wit_program_run_host(prog, po2, code.data(), W_CODE, got.data(), W_DATA);
                if (!fits) {
                    if (!e || !*e || got != data) {
                        printf("seed %u po2 %u: run_host took a sort that does not fit the shape, or wrote before it refused\n", seed, po2);
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
                for (const Sort& s : c.sorts) direct_sort(s, po2, want);
                for (const Count& ct : c.counts) direct_count(ct, po2, want);
                if (got != want) {
                    size_t k = 0;
                    while (got[k] == want[k]) ++k;
                    printf("seed %u po2 %u pattern %u: data[%zu][%zu] is %u by run_host, %u by the definition\n", seed, po2, kind, k / n, k % n, got[k], want[k]);
                    return 1;
                }
                for (uint32_t col = 0; col < W_DATA; ++col)  // every column the program does not write is as planted
                    if (!(col >= 4 && col < 6) && !written.count(col) && memcmp(&got[(size_t)col * n], &data[(size_t)col * n], 4 * (size_t)n)) {
                        printf("seed %u po2 %u: column %u is no dest and was written\n", seed, po2, col);
                        return 1;
                    }
                for (const Sort& s : c.sorts) {
                    const uint32_t rows = s.rows ? s.rows : n;
                    for (uint32_t q = 0; q < s.n_cols; ++q) {
                        for (uint32_t r = rows; r < n; ++r)
                            if (got[(size_t)s.dests[q] * n + r] != POISON) {
                                printf("seed %u po2 %u: row %u of dest %u is at or above rows = %u and was written\n", seed, po2, r, s.dests[q], rows);
                                return 1;
                            }
                        for (uint32_t r = 0; r < rows; ++r) moved += got[(size_t)s.dests[q] * n + r] != got[(size_t)s.sources[q] * n + r];
                    }
                    ++sorted;
                }
                ++ran;
            }
        bx_wit_program_destroy(prog);
    }
    printf("compiled %ld (of them malformed-but-valid %ld), refused %ld, runs %ld, refused for the shape %ld, sorts evaluated %ld, cells moved %ld\n", compiled,
           compiled_malformed, refused, ran, shape_refused, sorted, moved);
    if (compiled < 1500 || refused < 500 || ran < 5000 || shape_refused < 1000 || sorted < 5000 || moved < 5000) {
        printf("the case mix is too thin to mean anything\n");
        return 1;
    }
    printf("wit_sort_check ok\n");
    return 0;
}
