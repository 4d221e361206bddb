// p2_live_check.cpp — CPU check of the live range of the Poseidon2 permutation (boundless_amd/csrc/poseidon2_arith.hpp:
// poseidon2_mix_bounded<DIAG, LO, HI>, the host mirror of poseidon2.hip's poseidon2_mix<LO, HI>), compiled with -DBX_CHECK_BOUNDS so
// that every documented magnitude is asserted per value.  The ranged permutations <16, 24> (a sponge that absorbs again) and <0, 8>
// (the digest) are compared with the full one on their live cells, and the full one with the plain canonical implementation, over
// random states, the extreme words of tests/extreme_words.py and the extreme diagonals of tests/p2_paired_check.cpp; then a chained
// sponge built as hash_rows_kernel builds it (<16, 24> for every block of 16 columns but the last, <0, 8> for the last, padded with
// zeros) against the plain chained sponge.  Built and run by tests/test_p2_live_cpu.py under
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

static uint64_t rng_state = 0x13198A2E03707344ull;
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
// square root mod P (Tonelli-Shanks; P - 1 = 15 * 2^27); false if a is not a square
static bool sqrtm(uint32_t a, uint32_t* root) {
    if (a == 0) { *root = 0; return true; }
    if (powm(a, (P - 1) / 2) != 1) return false;
    const uint32_t Q = 15;
    uint32_t z = 2;
    while (powm(z, (P - 1) / 2) == 1) ++z;
    uint32_t M = 27, c = powm(z, Q), t = powm(a, Q), r = powm(a, (Q + 1) / 2);
    while (t != 1) {
        uint32_t i = 0, tt = t;
        while (tt != 1) tt = mulm(tt, tt), ++i;
        uint32_t b = c;
        for (uint32_t k = 0; k + i + 1 < M; ++k) b = mulm(b, b);
        M = i, c = mulm(b, b), t = mulm(t, c), r = mulm(r, b);
    }
    *root = r;
    return true;
}

// ---- the diagonals of tests/p2_paired_check.cpp: canonical entries ----
struct Diag {
    const char* name;
    uint32_t d[24];
};
static Diag g_diags[16];
static int g_ndiags = 0;
static void add_diag(const char* name, const uint32_t* d) {
    g_diags[g_ndiags].name = name;
    memcpy(g_diags[g_ndiags].d, d, sizeof g_diags[0].d);
    ++g_ndiags;
}
static int make_diags() {
    uint32_t d[24];
    add_diag("shipped", POSEIDON2_DIAG);
    for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < 24; ++i) d[i] = (uint32_t)(rnd64() % P);
        add_diag("random", d);
    }
    for (int i = 0; i < 24; ++i) d[i] = 0;
    add_diag("zeros", d);
    for (int i = 0; i < 24; ++i) d[i] = 1;
    add_diag("ones", d);
    for (int i = 0; i < 24; ++i) d[i] = P - 1;
    add_diag("minus ones", d);
    for (int i = 0; i < 24; ++i) d[i] = i % 3 == 0 ? 0 : i % 3 == 1 ? 1 : P - 1;
    add_diag("0, 1, P-1", d);
    // A_i = d R^2 centres to +-(P-1)/2, and the diagonal word d R of cell 0 likewise
    const uint32_t rinv = powm(MONT_ONE, P - 2), half_p = (P - 1) / 2, half_n = (P + 1) / 2;
    const uint32_t a_pos = mulm(half_p, mulm(rinv, rinv)), a_neg = mulm(half_n, mulm(rinv, rinv));
    REQUIRE(fp_centre(fp_mul(fp_encode(a_pos), R2)) == (i32)half_p && fp_centre(fp_mul(fp_encode(a_neg), R2)) == -(i32)half_p);
    for (int i = 0; i < 24; ++i) d[i] = a_pos;
    d[0] = mulm(half_p, rinv);
    add_diag("A = +(P-1)/2", d);
    for (int i = 0; i < 24; ++i) d[i] = a_neg;
    d[0] = mulm(half_n, rinv);
    add_diag("A = -(P-1)/2", d);
    for (int i = 0; i < 24; ++i) d[i] = (i & 1) ? a_pos : a_neg;
    add_diag("A = +-(P-1)/2", d);
    // E_i = d^2 R centres to +-((P-1)/2 - k), the largest magnitude that has square roots
    uint32_t roots[4];
    int nroots = 0;
    for (uint32_t k = 0; nroots == 0; ++k) {
        uint32_t r;
        if (!sqrtm(mulm(half_p - k, rinv), &r)) continue;
        for (uint32_t target : {half_p - k, half_n + k}) {
            REQUIRE(sqrtm(mulm(target, rinv), &r) && mulm(r, r) == mulm(target, rinv));
            roots[nroots++] = r;
            roots[nroots++] = P - r;
        }
    }
    for (int i = 0; i < 24; ++i) d[i] = roots[0];
    add_diag("E extreme", d);
    for (int i = 0; i < 24; ++i) d[i] = roots[i % nroots];
    add_diag("E extreme, all roots", d);
    return 0;
}

static void make_prm(uint32_t* prm, const uint32_t* rc, const uint32_t* d) {
    memset(prm, 0, 240 * sizeof(uint32_t));
    for (int i = 0; i < 213; ++i) prm[i] = (uint32_t)((uint64_t)(rc[i] % P) * p2_rc_scale(i) % P);
    for (int i = 0; i < 24; ++i) prm[216 + i] = fp_encode(d[i]);
}

// the extreme words of tests/extreme_words.py (EDGE): the centred magnitudes are largest at P/2 and P/2 + 1
static const uint32_t EDGE[] = {0, 1, P - 1, P / 2, P / 2 + 1, P / 2 - 1, MONT_ONE, P - MONT_ONE};
enum { N_PATTERNS = 7 };  // all_half, all_half1, alt_half, all_pm1, edge_mix, zeros, random
static uint32_t word(int pattern, size_t i) {
    switch (pattern) {
        case 0: return P / 2;
        case 1: return P / 2 + 1;
        case 2: return P / 2 + (uint32_t)(i & 1);
        case 3: return P - 1;
        case 4: return EDGE[rnd64() % 8];
        case 5: return 0;
        default: return (uint32_t)(rnd64() % P);
    }
}

// one state through the full and the two ranged permutations
static int check_state(const uint32_t* in, const uint32_t* prm, const HostPoseidon2& ref, const char* diag_name) {
    uint32_t plain[24], full[24], cap[24], dig[24];
    memcpy(plain, in, sizeof plain);
    memcpy(full, in, sizeof full);
    memcpy(cap, in, sizeof cap);
    memcpy(dig, in, sizeof dig);
    ref.mix_scalar(plain);
    poseidon2_mix_bounded<216>(full, prm);
    poseidon2_mix_bounded<216, 16, 24>(cap, prm);
    poseidon2_mix_bounded<216, 0, 8>(dig, prm);
    if (memcmp(plain, full, sizeof plain) != 0) {
        fprintf(stderr, "full permutation differs from the canonical one (diagonal '%s')\n", diag_name);
        return 1;
    }
    for (int i = 0; i < 24; ++i) {
        const uint32_t want_cap = i >= 16 ? full[i] : in[i], want_dig = i < 8 ? full[i] : in[i];  // dead cells keep their input words
        if (cap[i] != want_cap || dig[i] != want_dig) {
            fprintf(stderr, "cell %d: <16,24> gives %u (want %u), <0,8> gives %u (want %u) (diagonal '%s')\n", i, cap[i], want_cap, dig[i],
                    want_dig, diag_name);
            return 1;
        }
        REQUIRE(cap[i] < P && dig[i] < P);
    }
    return 0;
}

static int check_permutations(const Diag& dg, bool shipped_rc) {
    uint32_t rc[213];
    for (int i = 0; i < 213; ++i) rc[i] = shipped_rc ? POSEIDON2_RC[i] : (uint32_t)(rnd64() % P);
    HostPoseidon2 ref;
    ref.load(rc, dg.d);
    uint32_t prm[240];
    make_prm(prm, rc, dg.d);
    uint32_t in[24];
    for (int pattern = 0; pattern < N_PATTERNS; ++pattern)
        for (int t = 0; t < (pattern == 4 ? 200 : pattern == 6 ? 300 : 1); ++t) {
            for (int i = 0; i < 24; ++i) in[i] = word(pattern, (size_t)i);
            if (check_state(in, prm, ref, dg.name)) return 1;
        }
    return 0;
}

// hash_rows_kernel's sponge over one row: every block of 16 columns but the last hands on the capacity, the last the digest
static void sponge_live(uint32_t out[8], const uint32_t* elems, size_t cols, const uint32_t* prm) {
    uint32_t s[24];
    memset(s, 0, sizeof s);
    size_t c = 0;
    for (; c + 16 < cols; c += 16) {
        for (int i = 0; i < 16; ++i) s[i] = elems[c + i];
        poseidon2_mix_bounded<216, 16, 24>(s, prm);
    }
    for (int i = 0; i < 16; ++i) s[i] = c + i < cols ? elems[c + i] : 0u;
    poseidon2_mix_bounded<216, 0, 8>(s, prm);
    memcpy(out, s, 32);
}
// the plain chained sponge: the full permutation per block, a padded last block only where columns are left over (or there are none)
static void sponge_plain(uint32_t out[8], const uint32_t* elems, size_t cols, const uint32_t* prm) {
    uint32_t s[24];
    memset(s, 0, sizeof s);
    size_t c = 0;
    for (; c + 16 <= cols; c += 16) {
        for (int i = 0; i < 16; ++i) s[i] = elems[c + i];
        poseidon2_mix_bounded<216>(s, prm);
    }
    if (c < cols || cols == 0) {
        for (int i = 0; i < 16; ++i) s[i] = c + i < cols ? elems[c + i] : 0u;
        poseidon2_mix_bounded<216>(s, prm);
    }
    memcpy(out, s, 32);
}

static int check_sponges(const Diag& dg, bool shipped_rc) {
    uint32_t rc[213];
    for (int i = 0; i < 213; ++i) rc[i] = shipped_rc ? POSEIDON2_RC[i] : (uint32_t)(rnd64() % P);
    HostPoseidon2 ref;
    ref.load(rc, dg.d);
    uint32_t prm[240];
    make_prm(prm, rc, dg.d);
    const size_t col_counts[] = {0, 1, 15, 16, 17, 31, 32, 33, 48, 256};
    for (size_t cols : col_counts)
        for (int pattern = 0; pattern < N_PATTERNS; ++pattern) {
            std::vector<uint32_t> row(cols);  // exactly cols words: reading a column past the end is an AddressSanitizer error
            for (size_t i = 0; i < cols; ++i) row[i] = word(pattern, i);
            uint32_t a[8], b[8], c[8];
            sponge_live(a, row.data(), cols, prm);
            sponge_plain(b, row.data(), cols, prm);
            ref.hash_elems(c, row.data(), cols);
            if (memcmp(a, b, 32) != 0 || memcmp(a, c, 32) != 0) {
                fprintf(stderr, "sponge over %zu columns, pattern %d: live-range digest differs (diagonal '%s')\n", cols, pattern, dg.name);
                return 1;
            }
        }
    return 0;
}

int main() {
    if (make_diags()) return 1;
    for (int k = 0; k < g_ndiags; ++k) {
        if (check_permutations(g_diags[k], k == 0)) return 1;
        if (k == 0 && check_permutations(g_diags[k], false)) return 1;
        if (check_sponges(g_diags[k], k == 0)) return 1;
    }
    {   // published KAT through the ranged forms
        uint32_t prm[240], k[24];
        make_prm(prm, POSEIDON2_RC, POSEIDON2_DIAG);
        for (int i = 0; i < 24; ++i) k[i] = fp_encode((uint32_t)i);
        poseidon2_mix_bounded<216, 0, 8>(k, prm);
        REQUIRE(fp_decode(k[0]) == 0x2ed3e23du && fp_decode(k[1]) == 0x12921fb0u);
        for (int i = 0; i < 24; ++i) k[i] = fp_encode((uint32_t)i);
        poseidon2_mix_bounded<216, 16, 24>(k, prm);
        REQUIRE(fp_decode(k[23]) == 0x57a99864u);
    }
    printf("p2_live_check ok (%d diagonals)\n", g_ndiags);
    return 0;
}
