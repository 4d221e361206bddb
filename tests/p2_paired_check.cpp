// p2_paired_check.cpp — CPU check of the paired internal rounds of the Poseidon2 kernels (boundless_amd/csrc/poseidon2_arith.hpp:
// internal_round_pair), compiled with -DBX_CHECK_BOUNDS so that every documented magnitude is asserted per value.  One paired step
// is compared cell by cell (mod P) with two internal_round<false> calls, and the whole permutation (poseidon2_mix_bounded, the
// device's order and arithmetic) with the plain canonical implementation, over diagonals and cells chosen to reach the largest
// accumulators.  Built and run by tests/test_p2_paired_cpu.py, once more under -fsanitize=signed-integer-overflow,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static uint32_t res(i32 v) { return (uint32_t)(((i64)v % (i64)P + (i64)P) % (i64)P); }  // exact residue in [0, P)
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

// ---- the diagonals: canonical entries ----
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
    // A_i = d R^2 centres to +-(P-1)/2: d = target * R^-2; likewise the diagonal word d R itself (cell 0's multiplier)
    const uint32_t rinv = powm(MONT_ONE, P - 2), half_p = (P - 1) / 2, half_n = (P + 1) / 2;  // +(P-1)/2 and -(P-1)/2 as residues
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
    // E_i = d^2 R centres to +-(P-1)/2: d = sqrt(target * R^-1).  -1 is a square mod P, so +target and -target have roots
    // together or not at all: take the largest magnitude (P-1)/2 - k that has them (k is printed)
    uint32_t roots[4];
    int nroots = 0;
    for (uint32_t k = 0; nroots == 0; ++k) {
        uint32_t r;
        if (!sqrtm(mulm(half_p - k, rinv), &r)) continue;
        printf("E extreme: |E| = (P-1)/2 - %u\n", k);
        for (uint32_t target : {half_p - k, half_n + k}) {
            REQUIRE(sqrtm(mulm(target, rinv), &r) && mulm(r, r) == mulm(target, rinv));
            const uint32_t dm = fp_encode(r);
            REQUIRE(fp_centre(fp_mul(dm, dm)) == (target < half_n ? (i32)(half_p - k) : -(i32)(half_p - k)));
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

static int sgn(i32 v) { return v < 0 ? -1 : 1; }

// one paired step against two plain rounds
static int check_pair_once(const i32* x, const uint32_t* diag_m, const i32* E, const i32* A, const uint32_t* rc2, i32* out) {
    i32 a[24], b[24];
    memcpy(a, x, sizeof a);
    memcpy(b, x, sizeof b);
    internal_round<false>(a, diag_m, rc2);
    internal_round<false>(a, diag_m, rc2 + 1);
    internal_round_pair(b, E, A, rc2);
    for (int i = 0; i < 24; ++i) {
        if (res(a[i]) != res(b[i])) {
            fprintf(stderr, "paired step: cell %d is %d, two plain rounds give %d\n", i, b[i], a[i]);
            return 1;
        }
        REQUIRE(iabs64(b[i]) <= B_INT);
    }
    if (out) memcpy(out, b, sizeof b);
    return 0;
}

static int check_pairs(const Diag& dg) {
    uint32_t diag_m[24];
    i32 E[24], A[24];
    for (int i = 0; i < 24; ++i) diag_m[i] = fp_encode(dg.d[i]);
    p2_pair_consts(diag_m, E, A);
    for (int i = 0; i < 24; ++i) REQUIRE(iabs64(E[i]) <= B_K && iabs64(A[i]) <= B_K);
    for (int i = 1; i < 24; ++i) {  // E_i = d^2 R, A_i = d R^2 as residues
        REQUIRE(res(E[i]) == mulm(mulm(dg.d[i], dg.d[i]), MONT_ONE) && res(A[i]) == mulm(dg.d[i], mulm(MONT_ONE, MONT_ONE)));
    }
    REQUIRE(res(E[0]) == diag_m[0]);
    const uint32_t rcs[][2] = {{0, 0}, {P - 1, P - 1}, {P - 1, 0}, {1, P / 2}};
    const i32 B = (i32)B_INT;
    i32 x[24];
    // extreme cells: every cell at +-B_INT, signs per cell as sign(A_i) (largest dot-product groups), sign(E_i) (largest cell
    // operands), their negations, all of one sign, alternating; cell 0 with either sign; and zeros
    for (int mode = 0; mode < 9; ++mode)
        for (int s0 = -1; s0 <= 1; s0 += 2)
            for (const auto& rc2 : rcs) {
                for (int i = 0; i < 24; ++i) {
                    const int sg = mode == 0 ? sgn(A[i]) : mode == 1 ? -sgn(A[i]) : mode == 2 ? sgn(E[i]) : mode == 3 ? -sgn(E[i]) : mode == 4 ? 1
                                 : mode == 5 ? -1 : mode == 6 ? ((i & 1) ? 1 : -1) : mode == 7 ? sgn(A[i]) * sgn(E[i]) : 0;
                    x[i] = sg * B;
                }
                x[0] = mode == 8 ? 0 : s0 * B;
                if (check_pair_once(x, diag_m, E, A, rc2, nullptr)) return 1;
            }
    // chained pairs: the output of one step is the input of the next; one start in three has every cell at +-B_INT
    for (int chain = 0; chain < 300; ++chain) {
        for (int i = 0; i < 24; ++i) {
            const uint64_t r = rnd64();
            x[i] = chain % 3 == 0 ? ((r & 1) ? B : -B) : chain % 3 == 1 ? (i32)((i64)(r % (uint64_t)(2 * B_INT + 1)) - B_INT) : (i32)(r % P);
            if (chain % 3 == 2 && x[i] > B) x[i] -= (i32)P;  // canonical words, brought into the bound
        }
        for (int step = 0; step < 70; ++step) {
            const uint32_t rc2[2] = {(uint32_t)(rnd64() % P), (uint32_t)(rnd64() % P)};
            i32 y[24];
            if (check_pair_once(x, diag_m, E, A, rc2, y)) return 1;
            memcpy(x, y, sizeof x);
        }
    }
    return 0;
}

static int check_permutation(const Diag& dg, bool shipped) {
    uint32_t rc[213];
    for (int i = 0; i < 213; ++i) rc[i] = shipped ? POSEIDON2_RC[i] : (uint32_t)(rnd64() % P);
    HostPoseidon2 ref;
    ref.load(rc, dg.d);
    uint32_t prm[240];
    make_prm(prm, rc, dg.d);
    const uint32_t pool[] = {0, 1, 2, P - 1, P - 2, (P - 1) / 2, (P + 1) / 2, MONT_ONE};
    for (int t = 0; t < 600; ++t) {
        uint32_t a[24], b[24];
        for (int i = 0; i < 24; ++i) {
            const uint64_t r = rnd64();
            a[i] = t == 0 ? 0 : t == 1 ? P - 1 : t == 2 ? ((i & 1) ? (P - 1) / 2 : (P + 1) / 2) : t < 200 ? pool[r % 8] : (uint32_t)(r % P);
        }
        memcpy(b, a, sizeof a);
        ref.mix_scalar(a);
        poseidon2_mix_bounded<216>(b, prm);
        if (memcmp(a, b, sizeof a) != 0) {
            fprintf(stderr, "permutation mismatch: diagonal '%s', input %d\n", dg.name, t);
            return 1;
        }
    }
    return 0;
}

int main() {
    if (make_diags()) return 1;
    for (int k = 0; k < g_ndiags; ++k) {
        if (check_pairs(g_diags[k])) {
            fprintf(stderr, "  (diagonal '%s')\n", g_diags[k].name);
            return 1;
        }
        if (check_permutation(g_diags[k], k == 0)) return 1;
        if (k == 0 && check_permutation(g_diags[k], false)) return 1;
    }
    {   // published KAT through the paired form
        uint32_t prm[240], k[24];
        make_prm(prm, POSEIDON2_RC, POSEIDON2_DIAG);
        for (int i = 0; i < 24; ++i) k[i] = fp_encode((uint32_t)i);
        poseidon2_mix_bounded<216>(k, prm);
        REQUIRE(fp_decode(k[0]) == 0x2ed3e23du && fp_decode(k[1]) == 0x12921fb0u && fp_decode(k[23]) == 0x57a99864u);
    }
    printf("p2_paired_check ok (%d diagonals)\n", g_ndiags);
    return 0;
}
