// p2_rcfold_check.cpp — CPU check of the folded external round constants of the Poseidon2 permutation and of the signed carried
// capacity (boundless_amd/csrc/poseidon2_arith.hpp: p2_fold_consts, p2_build_table, sbox7s_n with K, sredc_all,
// poseidon2_mix_bounded<DIAG, LO, HI, SIGNED_OUT>, the host mirror of poseidon2.hip's poseidon2_mix), compiled with -DBX_CHECK_BOUNDS so
// that every documented magnitude is asserted per value.
//   * the table: words [0, 288) are what the builder before the folded region produced; in the region behind them blocks 3 and 7
//     are zero, every pair is {K, 0} with K canonical, and c = K * 2^-32 satisfies M c == rc' for rounds 1, 2, 3, 5, 6, 7 (M written
//     out as the 24 x 24 matrix circ(2 M4, M4, ..., M4), not through its inverse);
//   * the permutation: the bounded form against the plain canonical one over the full range, <16, 24>, <0, 8> and the signed
//     <16, 24> whose cells are canonical once reduced;
//   * the sponge as hash_rows_kernel chains it (signed <16, 24> for every block but the last, <0, 8> for the last) against the plain
//     one, for every column count 0..256;
// over extreme words (0, 1, P-1, all equal, the centred extremes) and random ones, with the built-in parameters and random ones, round
// constants all 0, all 1, all P-1, and extreme diagonals.  Built and run by tests/test_p2_rcfold_cpu.py under
// -fsanitize=address,undefined,signed-integer-overflow; a stand-alone program, never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fp.hpp"
#include "poseidon2_arith.hpp"
#include "poseidon2_params.hpp"
#include "transcript.hpp"

using namespace bx;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd64() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
#define REQUIRE(cond)                                                     \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__);    \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static uint32_t mulm(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)a * b % P); }
static uint32_t powm(uint32_t b, uint64_t e) {
    uint32_t r = 1;
    for (; e; e >>= 1, b = mulm(b, b))
        if (e & 1) r = mulm(r, b);
    return r;
}

// ---- parameter sets: canonical round constants and diagonal ----
struct Params {
    const char* name;
    uint32_t rc[213], d[24];
};
static std::vector<Params> g_params;
static void add_params(const char* name, const uint32_t* rc, const uint32_t* d) {
    Params p;
    p.name = name;
    memcpy(p.rc, rc, sizeof p.rc);
    memcpy(p.d, d, sizeof p.d);
    g_params.push_back(p);
}
static void make_params() {
    uint32_t rc[213], d[24];
    add_params("built-in", POSEIDON2_RC, POSEIDON2_DIAG);
    for (int k = 0; k < 3; ++k) {
        for (int i = 0; i < 213; ++i) rc[i] = (uint32_t)(rnd64() % P);
        for (int i = 0; i < 24; ++i) d[i] = (uint32_t)(rnd64() % P);
        add_params("random", rc, d);
    }
    const uint32_t consts[3] = {0u, 1u, P - 1};
    const char* names[3] = {"rc = 0", "rc = 1", "rc = P-1"};
    for (int k = 0; k < 3; ++k) {
        for (int i = 0; i < 213; ++i) rc[i] = consts[k];
        add_params(names[k], rc, POSEIDON2_DIAG);
    }
    for (int i = 0; i < 213; ++i) rc[i] = consts[rnd64() % 3];
    add_params("rc in {0, 1, P-1}", rc, POSEIDON2_DIAG);
    // extreme diagonals under random and under extreme constants
    for (int i = 0; i < 213; ++i) rc[i] = (uint32_t)(rnd64() % P);
    for (int i = 0; i < 24; ++i) d[i] = 0;
    add_params("diagonal 0", rc, d);
    for (int i = 0; i < 24; ++i) d[i] = 1;
    add_params("diagonal 1", rc, d);
    for (int i = 0; i < 24; ++i) d[i] = P - 1;
    add_params("diagonal P-1", rc, d);
    // A_i = d R^2 centres to +-(P-1)/2 in turn, and the diagonal word d R of cell 0 to +(P-1)/2 (tests/p2_live_check.cpp)
    const uint32_t rinv = powm(MONT_ONE, P - 2), half_p = (P - 1) / 2, half_n = (P + 1) / 2;
    for (int i = 0; i < 24; ++i) d[i] = mulm((i & 1) ? half_p : half_n, mulm(rinv, rinv));
    d[0] = mulm(half_p, rinv);
    for (int i = 0; i < 213; ++i) rc[i] = P - 1;
    add_params("A = +-(P-1)/2, rc = P-1", rc, d);
}

// the table as it was built before the folded region existed: 288 words
static void build_table_before(const uint32_t* rc, const uint32_t* d, uint32_t* h) {
    memset(h, 0, 288 * sizeof(uint32_t));
    for (int i = 0; i < 213; ++i) h[i] = (uint32_t)((uint64_t)(rc[i] % P) * p2_rc_scale(i) % P);
    for (int i = 0; i < 24; ++i) h[216 + i] = fp_encode(d[i]);
    i32 pe[24], pa[24];
    p2_pair_consts(h + 216, pe, pa);
    for (int i = 0; i < 24; ++i) h[240 + i] = (uint32_t)pe[i], h[264 + i] = (uint32_t)pa[i];
}

static int check_table(const Params& pm, const uint32_t* table) {
    uint32_t before[288];
    build_table_before(pm.rc, pm.d, before);
    REQUIRE(P2_TABLE_WORDS == 288 + 8 * 48 && P2_FOLD_OFF == 288 && P2_FOLD_OFF % 8 == 0);
    REQUIRE(memcmp(before, table, sizeof before) == 0);
    const uint32_t rinv = powm(MONT_ONE, P - 2);  // 2^-32 mod P
    for (int b = 0; b < 8; ++b) {
        const uint32_t* blk = table + 288 + 48 * b;
        if (b == 3 || b == 7) {
            for (int i = 0; i < 48; ++i) REQUIRE(blk[i] == 0u);
            continue;
        }
        const int round = b + 1;  // the external round whose constants the block carries: 1, 2, 3, 5, 6, 7
        const uint32_t* rcs = table + (round < 4 ? 24 * round : 117 + 24 * (round - 4));
        uint32_t c[24];
        for (int i = 0; i < 24; ++i) {
            REQUIRE(blk[2 * i] < P && blk[2 * i + 1] == 0u);
            c[i] = mulm(blk[2 * i], rinv);
        }
        static const uint32_t M4[4][4] = {{5, 7, 1, 3}, {4, 6, 1, 1}, {1, 3, 5, 7}, {1, 1, 4, 6}};
        for (int i = 0; i < 24; ++i) {  // row i of circ(2 M4, M4, ..., M4)
            uint64_t acc = 0;
            for (int j = 0; j < 24; ++j) acc += (uint64_t)M4[i & 3][j & 3] * (i / 4 == j / 4 ? 2u : 1u) * c[j];
            if ((uint32_t)(acc % P) != rcs[i]) {
                fprintf(stderr, "M c != rc' in round %d, cell %d (parameters '%s')\n", round, i, pm.name);
                return 1;
            }
        }
    }
    return 0;
}

// extreme words: the centred magnitudes are largest at P/2 and P/2 + 1 (tests/extreme_words.py)
static const uint32_t EDGE[] = {0, 1, P - 1, P / 2, P / 2 + 1, P / 2 - 1, MONT_ONE, P - MONT_ONE};
enum { N_PATTERNS = 9 };
static uint32_t word(int pattern, size_t i) {
    switch (pattern) {
        case 0: return 0;
        case 1: return 1;
        case 2: return P - 1;
        case 3: return P / 2;
        case 4: return P / 2 + 1;
        case 5: return P / 2 + (uint32_t)(i & 1);
        case 6: return EDGE[rnd64() % 8];
        case 7: return (i % 3 == 0) ? 0u : (i % 3 == 1) ? 1u : P - 1;
        default: return (uint32_t)(rnd64() % P);
    }
}
static uint32_t canon_word(uint32_t signed_word) {  // a carried cell -> the canonical word it stands for
    const int64_t v = (int32_t)signed_word;
    return (uint32_t)(((v % (int64_t)P) + (int64_t)P) % (int64_t)P);
}

static int check_state(const uint32_t* in, const uint32_t* table, const HostPoseidon2& ref, const char* name) {
    uint32_t plain[24], full[24], cap[24], dig[24], car[24];
    memcpy(plain, in, sizeof plain);
    memcpy(full, in, sizeof full);
    memcpy(cap, in, sizeof cap);
    memcpy(dig, in, sizeof dig);
    memcpy(car, in, sizeof car);
    ref.mix_scalar(plain);
    poseidon2_mix_bounded<216>(full, table);
    poseidon2_mix_bounded<216, 16, 24>(cap, table);
    poseidon2_mix_bounded<216, 0, 8>(dig, table);
    poseidon2_mix_bounded<216, 16, 24, true>(car, table);
    if (memcmp(plain, full, sizeof plain) != 0) {
        fprintf(stderr, "full permutation differs from the canonical one (parameters '%s')\n", name);
        return 1;
    }
    for (int i = 0; i < 24; ++i) {
        const uint32_t want_cap = i >= 16 ? full[i] : in[i], want_dig = i < 8 ? full[i] : in[i];  // dead cells keep their input words
        const uint32_t got_car = i >= 16 ? canon_word(car[i]) : car[i];
        if (cap[i] != want_cap || dig[i] != want_dig || got_car != want_cap) {
            fprintf(stderr, "cell %d: <16,24> %u, signed %u (want %u), <0,8> %u (want %u) (parameters '%s')\n", i, cap[i], got_car, want_cap,
                    dig[i], want_dig, name);
            return 1;
        }
        if (i >= 16) REQUIRE((int64_t)(int32_t)car[i] <= B_CARRY && (int64_t)(int32_t)car[i] >= -B_CARRY);
    }
    // the carried words feed a second permutation as they are: same result as from the canonical capacity
    uint32_t next_a[24], next_b[24];
    for (int i = 0; i < 24; ++i) next_a[i] = i < 16 ? in[(i + 5) % 16] : car[i], next_b[i] = i < 16 ? in[(i + 5) % 16] : cap[i];
    poseidon2_mix_bounded<216>(next_a, table);
    poseidon2_mix_bounded<216>(next_b, table);
    REQUIRE(memcmp(next_a, next_b, sizeof next_a) == 0);
    return 0;
}

// hash_rows_kernel's sponge over one row: every block of 16 columns but the last hands on the capacity as signed words, the last
// the canonical digest
static void sponge_carried(uint32_t out[8], const uint32_t* elems, size_t cols, const uint32_t* table) {
    uint32_t s[24];
    memset(s, 0, sizeof s);
    size_t c = 0;
    for (; c + 16 < cols; c += 16) {
        for (int i = 0; i < 16; ++i) s[i] = elems[c + i];
        poseidon2_mix_bounded<216, 16, 24, true>(s, table);
    }
    for (int i = 0; i < 16; ++i) s[i] = c + i < cols ? elems[c + i] : 0u;
    poseidon2_mix_bounded<216, 0, 8>(s, table);
    memcpy(out, s, 32);
}

static int check_sponges(const Params& pm, const uint32_t* table, const HostPoseidon2& ref, bool every_count) {
    static const size_t some[] = {0, 1, 15, 16, 17, 31, 32, 33, 48, 64, 256};
    std::vector<size_t> counts;
    if (every_count) for (size_t c = 0; c <= 256; ++c) counts.push_back(c);
    else counts.assign(some, some + sizeof some / sizeof some[0]);
    for (size_t cols : counts)
        for (int pattern = 0; pattern < N_PATTERNS; ++pattern) {
            if (every_count && pattern != 8 && pattern != 6 && cols % 16 > 1 && cols % 16 < 15) continue;  // the constant patterns: around the block edges
            std::vector<uint32_t> row(cols);  // exactly cols words: reading a column past the end is an AddressSanitizer error
            for (size_t i = 0; i < cols; ++i) row[i] = word(pattern, i);
            uint32_t a[8], b[8];
            sponge_carried(a, row.data(), cols, table);
            ref.hash_elems(b, row.data(), cols);
            if (memcmp(a, b, 32) != 0) {
                fprintf(stderr, "sponge over %zu columns, pattern %d: digest differs (parameters '%s')\n", cols, pattern, pm.name);
                return 1;
            }
            for (int i = 0; i < 8; ++i) REQUIRE(a[i] < P);
        }
    return 0;
}

int main() {
    make_params();
    for (size_t k = 0; k < g_params.size(); ++k) {
        const Params& pm = g_params[k];
        uint32_t table[P2_TABLE_WORDS];
        REQUIRE(p2_build_table(pm.rc, pm.d, table));
        if (check_table(pm, table)) return 1;
        HostPoseidon2 ref;
        ref.load(pm.rc, pm.d);
        uint32_t in[24];
        for (int pattern = 0; pattern < N_PATTERNS; ++pattern)
            for (int t = 0; t < (pattern == 6 ? 100 : pattern == 8 ? 150 : 1); ++t) {
                for (int i = 0; i < 24; ++i) in[i] = word(pattern, (size_t)i);
                if (check_state(in, table, ref, pm.name)) return 1;
            }
        if (check_sponges(pm, table, ref, k < 2)) return 1;  // every count 0..256 with the built-in and one random set
    }
    {   // the region the device reads is what the host mirror derives for itself from the stored constants
        uint32_t table[P2_TABLE_WORDS], fold[P2_FOLD_WORDS];
        REQUIRE(p2_build_table(POSEIDON2_RC, POSEIDON2_DIAG, table));
        REQUIRE(p2_fold_consts(table, fold) && memcmp(fold, table + P2_FOLD_OFF, sizeof fold) == 0);
    }
    {   // published KAT through the folded forms
        uint32_t table[P2_TABLE_WORDS], k[24];
        REQUIRE(p2_build_table(POSEIDON2_RC, POSEIDON2_DIAG, table));
        for (int i = 0; i < 24; ++i) k[i] = fp_encode((uint32_t)i);
        poseidon2_mix_bounded<216, 0, 8>(k, table);
        REQUIRE(fp_decode(k[0]) == 0x2ed3e23du && fp_decode(k[1]) == 0x12921fb0u);
        for (int i = 0; i < 24; ++i) k[i] = fp_encode((uint32_t)i);
        poseidon2_mix_bounded<216, 16, 24, true>(k, table);
        REQUIRE(fp_decode(canon_word(k[23])) == 0x57a99864u);
    }
    printf("p2_rcfold_check ok (%zu parameter sets)\n", g_params.size());
    return 0;
}
