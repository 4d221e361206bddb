/*
 * bx_groth16.h — the BN254 Groth16 prover ("shrink-wrap") of libbx_hip_hal.so, and its multi-scalar multiplications.
 *
 * Reference boundary this replaces
 * --------------------------------
 *   bento/crates/workflow/src/tasks/snark.rs:36-76      the snark task
 *   blake3_groth16/src/prove/cuda.rs:40-70              risc0_groth16_sys::prove(prover_params, setup_params)
 * Inputs are a snarkjs `.zkey` proving key and a witness (n_vars x 32-byte little-endian Fr elements, as circom_witnesscalc writes
 * them); the output is the snarkjs proof JSON.  INTEGRATION.md shows the Rust call sites.
 *
 * Conventions: those of bx_hal.h (NULL = ok, otherwise a message owned by the library; no call aborts and no exception crosses the
 * ABI).  The host-only calls that take no ctx (bx_groth16_zkey_inspect*, bx_groth16_*_json, and the whole verifier: bx_groth16_vk*,
 * bx_groth16_*_vk, bx_groth16_seal_*, bx_groth16_verify*, bx_bn254_pairing_check) return messages in a thread-local buffer, valid
 * until the next such call on the same thread; they need no GPU and may be called from several threads at once.  A key belongs to the ctx it was loaded on.  Numbers are 8 x u32
 * little-endian words; "canonical" means < the modulus and not in Montgomery form.  The file formats and encodings are stated in
 * boundless_amd/csrc/groth16.hpp and DESIGN.md §11.  bx_free releases the keys still loaded on its ctx.
 */
#ifndef BX_GROTH16_H
#define BX_GROTH16_H
#include <stddef.h>
#include <stdint.h>

#include "bx_hal.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BX_GROTH16_MAX_PUBLIC 64 /* public signals a proof carries (the blake3 circuit has 1, risc0's has 5) */
#define BX_GROTH16_MAX_DOMAIN_LOG 27 /* the odd coset needs a root of order 2N; Fr's two-adicity is 28 */
#define BX_BN254_MSM_MAX_N 267386880u /* 2^28 - 2^20 points per MSM; bx_groth16_key_load refuses keys whose MSMs would exceed it */

typedef struct bx_groth16_info {
    uint32_t n_vars;      /* witness length, including the constant 1 at index 0 */
    uint32_t n_public;    /* public signals: witness[1..n_public] */
    uint32_t domain_size; /* N: a power of two, at most 2^27 */
    uint64_t n_coefs;     /* records of the coefficient section (A and B) */
    uint64_t bytes;       /* size of the file */
} bx_groth16_info;

typedef struct bx_groth16_proof {
    uint32_t a[16]; /* A: x, y (canonical Fq) */
    uint32_t b[32]; /* B: x.c0, x.c1, y.c0, y.c1 */
    uint32_t c[16]; /* C: x, y */
    uint32_t n_public;
    uint32_t public_signals[BX_GROTH16_MAX_PUBLIC * 8]; /* witness[1..n_public], canonical Fr */
} bx_groth16_proof;

typedef struct bx_groth16_key bx_groth16_key;

/* Host only (no ctx, no GPU): parse and validate a zkey's header and section table.  Refuses a wrong magic, version or protocol, a
 * q or r other than BN254's, section sizes that do not match the header, a domain above 2^27 and truncated files. */
const char* bx_groth16_zkey_inspect(const char* path, bx_groth16_info* out);
const char* bx_groth16_zkey_inspect_mem(const void* bytes, size_t len, bx_groth16_info* out);

/* Parse, upload (chunked through pinned staging) and prepare a key on ctx: twiddles, the coefficient lists sorted by constraint
 * (CSR), every G1 / G2 point checked to have its coordinates below q (on the host, over the file's bytes: "... has a coordinate
 * not below q", naming the section) and to lie on its curve (those the prover uses on the device; IC and gamma2 on the host; no
 * subgroup check).  Refuses a key whose MSMs would exceed BX_BN254_MSM_MAX_N points.  Blocks. */
const char* bx_groth16_key_load(bx_ctx* ctx, const char* path, bx_groth16_key** out);
const char* bx_groth16_key_load_mem(bx_ctx* ctx, const void* bytes, size_t len, bx_groth16_key** out);
const char* bx_groth16_key_info(const bx_groth16_key* key, bx_groth16_info* out);
const char* bx_groth16_key_free(bx_ctx* ctx, bx_groth16_key* key);

/* One proof.  witness: n_vars x 32 bytes of canonical little-endian Fr with witness[0] == 1.  rs: NULL (r and s from OS randomness)
 * or 64 bytes, r then s, canonical little-endian.  Blocks until the proof is on the host. */
const char* bx_groth16_prove(bx_ctx* ctx, bx_groth16_key* key, const void* witness, size_t n_vars, const void* rs, bx_groth16_proof* out);

/* snarkjs JSON: {"pi_a": [x, y, "1"], "pi_b": [[x.c0, x.c1], [y.c0, y.c1], ["1", "0"]], "pi_c": [...], "protocol": "groth16",
 * "curve": "bn128"} with decimal strings; and the public signals as a JSON list of decimal strings. */
const char* bx_groth16_proof_json(const bx_groth16_proof* proof, char* buf, size_t cap);
const char* bx_groth16_public_json(const bx_groth16_proof* proof, char* buf, size_t cap);

/* sum scalars[i] * points[i] on device buffers (the prover's hot path).  points: affine, Montgomery form, little-endian, 16 words
 * per G1 point (x, y), 32 per G2 point (x.c0, x.c1, y.c0, y.c1), infinity as zeros.  Every coordinate must be below q and every
 * point on its curve: the hot path checks neither (bx_groth16_key_load does, for a key's points), and a coordinate stored as x + q
 * can give a wrong, fully reduced sum.  scalars: 8 words each; all 256 bits are read, so a scalar k that is not below r gives
 * (k mod r) * P, as the group law says — canonical scalars are not required (bx_groth16_prove checks its witness itself).  out
 * (host): the affine result in canonical coordinates (16 / 32 words), infinity as zeros.  n <= BX_BN254_MSM_MAX_N.  Blocks. */
const char* bx_bn254_msm_g1(bx_ctx* ctx, bx_buf points, bx_buf scalars, size_t n, uint32_t* out);
const char* bx_bn254_msm_g2(bx_ctx* ctx, bx_buf points, bx_buf scalars, size_t n, uint32_t* out);

/* ---- Verification: host only (no ctx, no GPU), what the reference's snark task does after proving
 * (bento/crates/workflow/src/tasks/snark.rs:58-59 and :76-78; blake3_groth16/src/verify.rs:63-77, verify_seal). ---- */

typedef struct bx_groth16_vk {
    uint32_t alpha1[16];                           /* G1: x, y (canonical Fq) */
    uint32_t beta2[32], gamma2[32], delta2[32];    /* G2: x.c0, x.c1, y.c0, y.c1 */
    uint32_t n_public;
    uint32_t ic[(BX_GROTH16_MAX_PUBLIC + 1) * 16]; /* IC_0 .. IC_n_public */
} bx_groth16_vk;

/* The verifying key a proving key carries (zkey section 2: alpha1, beta2, gamma2, delta2; section 3: IC).  The zkey readers refuse
 * what bx_groth16_zkey_inspect refuses and read sections 2 and 3 only.  Every way of building a vk checks that its coordinates are
 * below q, that alpha1, beta2, gamma2, delta2 and every IC lie on their curves, and that the three G2 points are not infinity and
 * lie in the subgroup of order r; n_public is at most BX_GROTH16_MAX_PUBLIC.  bx_groth16_key_vk answers from what
 * bx_groth16_key_load kept on the host: no device access. */
const char* bx_groth16_zkey_vk(const char* path, bx_groth16_vk* out);
const char* bx_groth16_zkey_vk_mem(const void* bytes, size_t len, bx_groth16_vk* out);
const char* bx_groth16_key_vk(const bx_groth16_key* key, bx_groth16_vk* out);

/* snarkjs verification_key.json: {"protocol": "groth16", "curve": "bn128", "nPublic": n, "vk_alpha_1": [x, y, "1"], "vk_beta_2":
 * [[x.c0, x.c1], [y.c0, y.c1], ["1", "0"]], "vk_gamma_2", "vk_delta_2", "IC": [[x, y, "1"], ...]} with decimal strings.
 * vk_alphabeta_12 is not written; it and every unknown key are ignored when read.  bx_groth16_proof_from_json reads what
 * bx_groth16_proof_json and bx_groth16_public_json write. */
const char* bx_groth16_vk_json(const bx_groth16_vk* vk, char* buf, size_t cap);
const char* bx_groth16_vk_from_json(const char* json, size_t len, bx_groth16_vk* out);
const char* bx_groth16_proof_from_json(const char* proof_json, size_t proof_len, const char* public_json, size_t public_len,
                                       bx_groth16_proof* out);

/* The on-chain seal: [4-byte selector] A.x A.y B.x.c1 B.x.c0 B.y.c1 B.y.c0 C.x C.y, 32 bytes big-endian each.  Decoding takes 260
 * bytes (the selector is skipped) or 256 (no selector), leaves n_public = 0 and checks nothing about the numbers: verification does. */
const char* bx_groth16_seal_encode(const bx_groth16_proof* proof, const uint8_t selector[4], uint8_t out[260]);
const char* bx_groth16_seal_decode(const uint8_t* seal, size_t len, bx_groth16_proof* out);

/* e(-A, B) e(alpha1, beta2) e(IC_0 + sum x_i IC_i, gamma2) e(C, delta2) = 1, by one multi-Miller loop and one final exponentiation.
 * NULL = accepted; otherwise the first failed check by name.  Strict, as the on-chain verifier is: a coordinate not below q, a
 * public signal not below r, proof.n_public != vk.n_public, A, B or C at infinity or off its curve and B outside the subgroup of
 * order r are refused as such; a well-formed proof that fails the equation gives "pairing check failed".  vk: from one of the
 * builders above (verification re-checks its ranges and curves, not its subgroups). */
const char* bx_groth16_verify(const bx_groth16_vk* vk, const bx_groth16_proof* proof);
/* The reference's verify_seal: one public input, claim_digest read as a big-endian number and reduced mod r. */
const char* bx_groth16_verify_seal(const bx_groth16_vk* vk, const uint8_t* seal, size_t len, const uint8_t claim_digest[32]);

/* prod e(g1[i], g2[i]) == 1 (the EIP-197 question).  g1: n x 16 words, g2: n x 32 words, canonical affine, infinity as zeros (such
 * a pair contributes 1); points off their curve or outside the subgroup are refused.  n = 0 is accepted.  NULL = yes. */
const char* bx_bn254_pairing_check(const uint32_t* g1, const uint32_t* g2, size_t n);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
