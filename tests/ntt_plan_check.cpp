// ntt_plan_check.cpp — the NTT planner (csrc/ntt_plan.hpp) without a GPU; stand-alone, built with -fsanitize=address,undefined by
// tests/test_ntt_plan_check_cpu.py.
//
//   ntt_plan_check <cases.txt>
//
// 1. Replay.  cases.txt is tests/golden/ntt_launches.json (the launches a kernel trace recorded on an MI355X, tools/ntt_launch_trace.py)
//    as lines.  For every case the entry point's sequence of planned launches must equal the recorded one: kernel (family and template
//    geometry), workgroup size and grid.  (The trace reports no dynamic LDS, so LDS is checked in part 2 only.)  Every row of
//    NTT_GEOMS must occur.
// 2. Properties, for every m in 1 .. 26 and every value of every ntt_* tunable in its range (the full product), with the remaining
//    arguments of ntt_plan (direction, expand / skip bits, columns, alignment, post-factor) drawn DRAWS times per combination from a
//    fixed seed: a plan or a known refusal comes back; no tile exceeds its kernel's launch bound; the radix-16 pass B has
//    10 <= m_lo + lt <= 14; threads and LDS bytes follow the formulas the launch sites had before the planner existed, restated here.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "ntt_plan.hpp"

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

struct Launch {
    std::string kernel;
    unsigned wg, gx, gy;
    bool operator==(const Launch& o) const { return kernel == o.kernel && wg == o.wg && gx == o.gx && gy == o.gy; }
};

static bool geom_seen[NTT_GEOM_COUNT];

static Launch planned(const NttPass& p, bool inv, bool pass_a, int skip) {
    char name[96];
    const char* b = inv ? "true" : "false";
    if (p.family == NTT_V1) {
        snprintf(name, sizeof name, "%s<%s>", pass_a ? "ntt_block_kernel" : "ntt_strided_kernel", b);
    } else if (p.family == NTT_MULTI_A) {
        snprintf(name, sizeof name, "ntt_passA_fwd12_multi_kernel<%d>", skip);
    } else {
        const NttGeom& g = NTT_GEOMS[p.geom];
        geom_seen[p.geom] = true;
        snprintf(name, sizeof name, "ntt_r16_kernel<%s, %s, %d, %d, %d, %d>", b, pass_a ? "true" : "false", skip, g.lr, g.lt, g.maxt);
    }
    return Launch{name, p.threads, p.grid_x, p.grid_y};
}

// the launches of one entry point, in stream order (ntt.hip: forward = per group A then B, inverse = B then A, then the unfused zk_shift)
static std::vector<Launch> entry_launches(const NttTunables& t, const std::string& entry, int m, size_t count, int bits, size_t offset) {
    std::vector<Launch> out;
    const bool al = offset % 4 == 0;
    if (entry == "interpolate" || entry == "interpolate_zk") {
        const bool zk = entry == "interpolate_zk";
        const NttPlan p = ntt_plan(t, true, m, 0, 0, count, al, zk && m >= 12);
        CHECK(!p.error, "%s", p.error);
        if (p.error) return out;
        if (p.m_lo) out.push_back(planned(p.b, true, false, 0));
        out.push_back(planned(p.a, true, true, 0));
        if (zk && !p.post_on_a) {
            size_t blocks = ((count << m) + 255) / 256;
            out.push_back(Launch{"zk_shift_kernel", 256, (unsigned)(blocks > 16384 ? 16384 : blocks), 1});
        }
        return out;
    }
    const int expand = entry == "expand" ? bits : 0, skip = bits;
    const size_t g = ntt_forward_group(t, m, expand, skip, count, al);
    for (size_t c0 = 0; c0 < count; c0 += g) {
        const NttPlan p = ntt_plan(t, false, m, expand, skip, count - c0 < g ? count - c0 : g, al, false);
        CHECK(!p.error, "%s", p.error);
        if (p.error) return out;
        out.push_back(planned(p.a, false, true, skip));
        if (p.m_lo) out.push_back(planned(p.b, false, false, 0));
    }
    return out;
}

static int replay(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) {
        printf("cannot open %s\n", path);
        return -1;
    }
    int cases = 0;
    char entry[32], line[256];
    NttTunables t;
    int m, bits, n;
    unsigned long count, offset;
    while (fscanf(f, " case %ld %ld %ld %ld %ld %ld %ld %ld %31s %d %lu %d %lu %d", &t.block_log, &t.tile_log, &t.fast, &t.tile_a_log, &t.tile_b_log,
                  &t.cols_per_wg, &t.group_cols, &t.tile_b_wide, entry, &m, &count, &bits, &offset, &n) == 14) {
        std::vector<Launch> want;
        for (int i = 0; i < n; ++i) {
            Launch l;
            if (fscanf(f, " %u %u %u %255[^\n]", &l.wg, &l.gx, &l.gy, line) != 4) {
                printf("case %d: malformed launch line\n", cases);
                fclose(f);
                return -1;
            }
            l.kernel = line;
            want.push_back(l);
        }
        const std::vector<Launch> got = entry_launches(t, entry, m, count, bits, offset);
        CHECK(got.size() == want.size(), "case %d (%s m=%d count=%lu): %zu planned launches, %zu recorded", cases, entry, m, count, got.size(), want.size());
        for (size_t i = 0; i < got.size() && i < want.size(); ++i)
            CHECK(got[i] == want[i], "case %d (%s m=%d count=%lu bits=%d offset=%lu) launch %zu: planned %s wg %u grid %u x %u, recorded %s wg %u grid %u x %u",
                  cases, entry, m, count, bits, offset, i, got[i].kernel.c_str(), got[i].wg, got[i].gx, got[i].gy, want[i].kernel.c_str(), want[i].wg,
                  want[i].gx, want[i].gy);
        ++cases;
    }
    fclose(f);
    for (int i = 0; i < NTT_GEOM_COUNT; ++i) CHECK(geom_seen[i], "row %d of NTT_GEOMS occurs in no recorded case", i);
    return cases;
}

// ---- properties ------------------------------------------------------------------------------------------------------------
static const char* const REFUSALS[] = {"ntt: size too large", "ntt: expand_bits larger than the block pass", "ntt: too many workgroups in one launch",
                                       "ntt: tile larger than the kernel's launch bound",
                                       "ntt: a column of 2^30 words or more does not fit pass B's 32-bit buffer offsets"};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;  // fixed seed (splitmix64)
static uint64_t draw() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void check_r16(const NttPass& p, bool pass_a, size_t count) {
    CHECK(p.geom >= 0 && p.geom < NTT_GEOM_COUNT, "geom %d", p.geom);
    if (p.geom < 0 || p.geom >= NTT_GEOM_COUNT) return;
    const NttGeom& g = NTT_GEOMS[p.geom];
    CHECK(g.pass_a == pass_a, "row %d is of the other pass", p.geom);
    CHECK((p.family == NTT_R16_GEOM) == (g.lr != 0), "family %d row %d", (int)p.family, p.geom);
    if (g.lr) CHECK(g.lr == p.lr && g.lt == p.lt, "row %d (%d, %d) for lr %d lt %d", p.geom, g.lr, g.lt, p.lr, p.lt);
    const uint32_t tile = 1u << (p.lrows + p.lt);
    CHECK(p.threads == tile / 16 && p.threads >= 64 && p.threads <= (uint32_t)g.maxt, "threads %u, tile %u, bound %d", p.threads, tile, g.maxt);
    CHECK(p.lds == ((size_t)tile + tile / 16) * 4, "lds %zu", p.lds);
    CHECK(p.grid_y == 1 && (size_t)p.grid_x == (size_t)p.tiles * count && (size_t)p.tiles * count < ((size_t)1 << 31), "grid %u", p.grid_x);
}

static void check_plan(const NttTunables& t, const NttPlan& p, bool inv, int m, int expand, int skip, size_t count, bool al, bool post) {
    if (p.error) {
        bool known = false;
        for (const char* r : REFUSALS) known = known || !strcmp(r, p.error);
        CHECK(known, "unknown refusal '%s'", p.error);
        return;
    }
    CHECK(p.m_hi >= 1 && p.m_hi <= TW_LOG && p.m_lo >= 0 && p.m_lo <= TW_LOG && p.m_hi + p.m_lo == m, "split %d + %d of %d", p.m_hi, p.m_lo, m);
    CHECK(p.twist == (p.m_lo != 0) && p.count == count, "twist / count");
    CHECK(p.a.family != NTT_ABSENT && (p.b.family == NTT_ABSENT) == (p.m_lo == 0), "families %d %d", (int)p.a.family, (int)p.b.family);
    CHECK(t.fast || (!p.a.r16() && !p.b.r16()), "ntt_fast = 0 plans a radix-16 pass");
    CHECK(!p.post_on_a || (inv && post && p.a.r16() && p.m_hi >= 4), "post_on_a");
    // pass A
    CHECK(p.a.lr == p.m_hi && p.a.lt == 0 && p.a.row_shift == 0, "pass A geometry");
    if (p.a.family == NTT_V1) {  // the launch site of ntt_block_kernel as it was
        const unsigned R = 1u << p.m_hi;
        const unsigned threads = R / 2 < 64 ? 64 : (R / 2 > 256 ? 256 : R / 2);
        CHECK(p.a.threads == threads && p.a.lds == (size_t)R * 8, "v1 pass A: threads %u lds %zu", p.a.threads, p.a.lds);
        CHECK(p.a.grid_x == 1u << p.m_lo && p.a.grid_y == (unsigned)count, "v1 pass A grid");
    } else {
        CHECK(al && (skip == 0 || (skip == 2 && !inv)) && (((size_t)1 << m) >> expand) % 4 == 0, "radix-16 pass A on a shape it does not cover");
        CHECK(p.a.lrows >= 10 && p.a.lrows >= p.a.lr && p.a.lrows <= m && p.a.tiles == 1u << (m - p.a.lrows), "pass A tile 2^%d", p.a.lrows);
        CHECK(p.a.lr != 13 || p.a.lrows == 13, "a 2^13 pass A on a tile of 2^%d", p.a.lrows);
        if (p.a.family == NTT_MULTI_A) {  // __launch_bounds__(256, 1), two 2^12 tiles
            CHECK(!inv && p.a.lr == 12 && p.a.lrows == 12 && count > 1 && p.a.cpw > 1 && p.a.cpw == (uint32_t)t.cols_per_wg && (expand == 0 || expand == 2),
                  "multi-column pass A on a shape it does not cover");
            CHECK(p.a.threads == 256 && p.a.lds == (4096 + 256) * 4 * 2, "multi-column pass A: threads %u lds %zu", p.a.threads, p.a.lds);
            CHECK(p.a.grid_y == 1 && p.a.grid_x == p.a.tiles * (uint32_t)((count + p.a.cpw - 1) / p.a.cpw), "multi-column pass A grid");
        } else {
            check_r16(p.a, true, count);
        }
    }
    if (!p.m_lo) return;
    // pass B
    CHECK(p.b.lr == p.m_lo && p.b.lrows == p.m_lo && p.b.row_shift == p.m_hi && p.b.lt >= 0 && p.b.lt <= p.m_hi && p.b.tiles == 1u << (p.m_hi - p.b.lt),
          "pass B geometry");
    if (p.b.family == NTT_V1) {  // the launch site of ntt_strided_kernel as it was, with the tile of ntt_tile_log
        int tile = (int)t.tile_log;
        if (tile < p.m_lo) tile = p.m_lo;
        int lt = tile - p.m_lo;
        if (lt > p.m_hi) lt = p.m_hi;
        const unsigned rows = 1u << p.m_lo, total = rows << lt;
        unsigned threads = total / 2 > 1024 ? 1024 : (total / 2 < 64 ? 64 : total / 2);
        if (threads > 512 && total <= 8192) threads = 512;
        CHECK(p.b.lt == lt && p.b.threads == threads && p.b.lds == (size_t)total * 4 + (size_t)rows * 4, "v1 pass B: lt %d threads %u lds %zu", p.b.lt,
              p.b.threads, p.b.lds);
        CHECK(p.b.grid_x == 1u << (p.m_hi - lt) && p.b.grid_y == (unsigned)count, "v1 pass B grid");
    } else {
        CHECK(p.m_lo + p.b.lt >= 10 && p.m_lo + p.b.lt <= 14, "radix-16 pass B on a tile of 2^%d", p.m_lo + p.b.lt);
        check_r16(p.b, false, count);
    }
    CHECK(p.a.lds <= 160 * 1024 && p.b.lds <= 160 * 1024, "LDS beyond a workgroup's 160 KiB");
}

static long properties() {
    static const int BITS[][2] = {{0, 0}, {0, 1}, {0, 2}, {0, 3}, {1, 1}, {2, 2}, {3, 3}, {0, 13}, {14, 14}};  // {expand, skip}
    static const size_t COUNTS[] = {1, 2, 3, 5, 16, 17, 256, 4096, (size_t)1 << 20};
    const int DRAWS = 4;
    long plans = 0;
    NttTunables t;
    for (int m = 1; m <= 26; ++m)
        for (t.block_log = 1; t.block_log <= 13; ++t.block_log)
            for (t.tile_log = 6; t.tile_log <= 15; ++t.tile_log)
                for (t.fast = 0; t.fast <= 1; ++t.fast)
                    for (t.tile_a_log = 10; t.tile_a_log <= 13; ++t.tile_a_log)
                        for (t.tile_b_log = 10; t.tile_b_log <= 14; ++t.tile_b_log)
                            for (t.cols_per_wg = 1; t.cols_per_wg <= 16; ++t.cols_per_wg)
                                for (t.tile_b_wide = 0; t.tile_b_wide <= 1; ++t.tile_b_wide)
                                    for (int d = 0; d < DRAWS; ++d) {
                                        const uint64_t r = draw();
                                        const bool inv = r & 1, al = (r >> 1) & 3, post = (r >> 3) & 1;  // aligned three times in four
                                        const int* b = BITS[(r >> 8) % (sizeof BITS / sizeof BITS[0])];
                                        const size_t count = COUNTS[(r >> 16) % (sizeof COUNTS / sizeof COUNTS[0])];
                                        const int expand = inv ? 0 : b[0], skip = inv ? 0 : b[1];
                                        check_plan(t, ntt_plan(t, inv, m, expand, skip, count, al, post), inv, m, expand, skip, count, al, post);
                                        ++plans;
                                    }
    // ntt_group_cols only chooses the columns per round: the whole range at the sizes and counts where rounds can differ
    t = NttTunables();
    for (int m = 10; m <= 26; ++m)
        for (t.group_cols = 0; t.group_cols <= 4096; ++t.group_cols)
            for (size_t count : COUNTS)
                for (int al = 0; al <= 1; ++al) {
                    const size_t g = ntt_forward_group(t, m, 2, 2, count, al);
                    const NttPlan p = ntt_plan(t, false, m, 2, 2, g, al, false);
                    CHECK(g == count || (g == (size_t)t.group_cols && g < count && (p.error || (p.a.r16() && p.b.r16()))), "group of %zu for %zu columns", g, count);
                    ++plans;
                }
    // beyond the tables: refused, not planned
    for (int m = 27; m <= 40; ++m) {
        const NttPlan p = ntt_plan(NttTunables(), m & 1, m, 0, 0, 1, true, false);
        CHECK(p.error && !strcmp(p.error, REFUSALS[0]), "2^%d is planned", m);
    }
    return plans;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: ntt_plan_check <cases.txt>\n");
        return 2;
    }
    const int cases = replay(argv[1]);
    if (cases <= 0) return 1;
    const long plans = properties();
    printf("%d recorded cases replayed, %ld plans checked, %ld failures\n", cases, plans, failures);
    if (failures) return 1;
    printf("ntt_plan_check ok\n");
    return 0;
}
