// groth16.hpp — internal state of a Groth16 proving key (include/bx_groth16.h) and the conventions of the prover, in one place.
//
// PINNED by the reference vector (tests/golden/groth16/blake3_groth16_reference.json, checked by tests/test_groth16_cpu.py):
//   * q = 21888242871839275222246405745257275088696311157297823662689037894645226208583 (Fq),
//     r = 21888242871839275222246405745257275088548364400416034343698204186575808495617 (Fr);
//   * G1: y^2 = x^3 + 3 over Fq; G2 on the twist y^2 = x^3 + 3/(9+u) over Fq2 = Fq[u]/(u^2+1);
//   * the on-chain seal: a 4-byte selector, then A.x, A.y, B.x.c1, B.x.c0, B.y.c1, B.y.c0, C.x, C.y, each 32 bytes big-endian
//     (imaginary part first: the EIP-197 order);
//   * verification: e(-A, B) e(alpha1, beta2) e(IC0 + sum x_i IC_i, gamma2) e(C, delta2) = 1.
// RECALLED from snarkjs / rapidsnark, not checkable without a real key (tests/test_groth16_upstream.py checks a real zkey + wtns
// when they are placed under tests/golden/groth16/upstream/):
//   1. zkey layout: "zkey", u32 version 1, u32 section count; each section is u32 type, u64 size, data.  1: u32 protocol (1 =
//      Groth16).  2: u32 n8q, q, u32 n8r, r, u32 nVars, u32 nPublic, u32 domainSize, alpha1, beta1, beta2, gamma2, delta1, delta2.
//      3: IC (nPublic + 1 G1).  4: u32 count, then records (u32 matrix, u32 constraint, u32 signal, 32-byte value).  5: A, 6: B1
//      (G1), 7: B2 (G2), nVars points each.  8: C (nVars - nPublic - 1 G1).  9: H (domainSize G1).  10: contributions (ignored).
//   2. q and r are canonical little-endian; points are affine, little-endian, Montgomery form (R = 2^256), G2 as x.c0, x.c1, y.c0,
//      y.c1; infinity is all zeros.
//   3. coefficient values are stored as c * R^2 mod r: one Montgomery product with a canonical witness value gives c * w in
//      Montgomery form.  The coefficient list carries the extra A-rows of the public signals (constraint nConstraints + i, signal i).
//   4. the H section is indexed by the odd coset: p_j = (A B - C)(omega_2N^(2j+1)), natural order j, with
//      omega_(2^k) = 5^((r-1)/2^k) mod r.
// The proof, with r and s:  A = alpha1 + sum w_i A_i + r delta1;  B2 = beta2 + sum w_i B2_i + s delta2;  B1 = beta1 + sum w_i B1_i +
// s delta1;  C = sum_{i > nPublic} w_i C_i + sum_j p_j H_j + s A + r B1 - r s delta1.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/bx_groth16.h"

namespace bx {

// a parsed zkey (host view into the caller's bytes; nothing copied)
struct ZkeyView {
    bx_groth16_info info{};
    const uint8_t* sec[11] = {};  // section data, by type (1..10); null = absent
    uint64_t sec_len[11] = {};
};
// validates everything bx_groth16_zkey_inspect promises; returns NULL or a message (written to err)
const char* zkey_parse(const uint8_t* p, size_t len, ZkeyView* out, char* err, size_t cap);
// bx_free: release the keys still loaded on a ctx (bn254.hip keeps the registry)
void groth16_release_keys(bx_ctx* c);

}  // namespace bx

struct bx_groth16_key {
    bx_ctx* ctx = nullptr;
    bx_groth16_info info{};
    uint32_t n_c = 0;  // points of section 8
    // device, Montgomery affine points.  The fixed terms of each sum ride along as extra points, so that one MSM computes each of
    // A, B2, B1 and C: A = [A_i..., alpha1, delta1], B1 = [B1_i..., beta1, delta1], B2 = [B2_i..., beta2, delta2],
    // CH = [C_i..., H_j..., A, B1, delta1] (A and B1 are written per proof).
    uint32_t *d_a = nullptr, *d_b1 = nullptr, *d_b2 = nullptr, *d_ch = nullptr;
    // NTT twiddles omega_N^k and omega_N^-k, k < N/2 (Fr, Montgomery)
    uint32_t *d_tw = nullptr, *d_itw = nullptr;
    // coefficient lists by constraint (CSR): row pointers (N + 1), signals, values (c R^2 mod r); A then B
    uint32_t *d_rows[2] = {}, *d_sig[2] = {}, *d_val[2] = {};
    // per-proof work: scalars of the four MSMs, the three polynomials
    uint32_t *d_sa = nullptr, *d_sb = nullptr, *d_sc = nullptr, *d_poly = nullptr;
    void* h_pin = nullptr;     // pinned staging of the key's uploads (Stager in bn254.hip), pin_bytes long
    size_t pin_bytes = 0;
    uint32_t omega2n_mont[8];  // omega_2N (coset generator), Montgomery
    uint32_t ninv_mont[8];     // 1/N, Montgomery
    std::vector<void*> allocs;
    // host copies of zkey sections 2 (header) and 3 (IC), as the file holds them: what bx_groth16_key_vk answers from
    std::vector<uint8_t> vk_header, vk_ic;
};
