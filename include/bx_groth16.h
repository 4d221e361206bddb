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
 * ABI).  The host-only calls that take no ctx (bx_groth16_zkey_inspect*, bx_groth16_*_json) return messages in a thread-local
 * buffer, valid until the next such call on the same thread.  A key belongs to the ctx it was loaded on.  Numbers are 8 x u32
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
 * (CSR), every G1 / G2 point checked to lie on its curve (those the prover uses on the device; IC and gamma2 on the host; no
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
 * per G1 point (x, y), 32 per G2 point (x.c0, x.c1, y.c0, y.c1), infinity as zeros; scalars: 8 words each, canonical.  out (host):
 * the affine result in canonical coordinates (16 / 32 words), infinity as zeros.  n <= BX_BN254_MSM_MAX_N.  Blocks. */
const char* bx_bn254_msm_g1(bx_ctx* ctx, bx_buf points, bx_buf scalars, size_t n, uint32_t* out);
const char* bx_bn254_msm_g2(bx_ctx* ctx, bx_buf points, bx_buf scalars, size_t n, uint32_t* out);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
