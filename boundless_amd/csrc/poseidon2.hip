// poseidon2.hip — Poseidon2 (BabyBear, t=24, rate 16, 4+21+4 rounds, x^7) Merkle hashing for gfx950.
//
// Restates risc0_zkp::hal::Hal::{hash_rows, hash_fold} with the `poseidon2` hash suite and
// risc0_zkp::core::hash::poseidon2::{poseidon2_mix, unpadded_hash} (risc0-zkp 3.0.3, reference Cargo.lock:9155),
// reached from bento/crates/workflow/src/tasks/prove.rs:41-49 via MerkleTreeProver::new.
//
// MI355X design: the permutation is pure 32-bit integer VALU work (~1.4k Montgomery products per
// 64 absorbed bytes) — no MFMA shape exists for it and it is nowhere near HBM-bound, so the kernel is organised
// around registers, not memory: one matrix row per lane, the 24-word state in VGPRs for the whole sponge,
// round constants fetched through wave-uniform (scalar) loads, loads of the column-major matrix coalesced
// across the 64 lanes of a wave (lane r reads matrix[c*rows + r]).
#include "ctx.hpp"
#include "poseidon2_arith.hpp"
#include "hash_suite.hpp"
#include "../../include/bx_image.h"

namespace bx {

constexpr int CELLS = 24, RATE = 16, RF_HALF = 4, RP = 21;
constexpr int DIAG_OFF = P2_DIAG_OFF;  // diagonal starts 32-byte aligned in the device parameter table (it and the tables behind it are read by 32-byte scalar loads)
constexpr int PAIR_OFF = P2_PAIR_OFF;  // behind it: the paired rounds' E[24], A[24] (centred)
constexpr int FOLD_OFF = P2_FOLD_OFF, P2_TABLE = P2_TABLE_WORDS;  // behind them: the folded external constants, eight blocks of 24 pairs {K, 0}

// ---------------------------------------------------------------------------------------------------------------
// Instruction budget.  The kernel is VALU-issue-bound and on gfx950 a 32-bit multiply-class op (v_mad_[iu]64_[iu]32,
// v_mul_lo/hi_u32, v_min_u32, v_lshl_add_u64) costs ~1.9 ns per wave and SIMD and a plain add/sub/and/mov ~1.05 ns
// (profiles/r01_microbench2_instr_cost.jsonl).  The permutation is organised to minimise that weighted instruction count,
// not multiplications (every bound below is asserted on the host by tests/host_arith_check.cpp, which compiles
// poseidon2_arith.hpp for the CPU and compares the whole permutation with the plain canonical implementation):
//   * cells are SIGNED 32-bit integers, only bounded in magnitude: the signed Montgomery reduction maps |t| <= 1.2 P^2 to
//     |r| < |t|/2^32 + P/2, so products of cells stay below 0.95 P by themselves and the permutation contains no
//     conditional subtraction at all except for the 24 words that leave it;
//   * linear layers run UNREDUCED in 64 bits (v_mad_i64_i32 multiplies by the small matrix entries and accumulates in one
//     instruction; external-layer outputs < 2^38, internal-layer sum < 2^37);
//   * the return to 32 bits is one bare REDC per cell, x = REDC(y + rc') [REDC = * 2^-32 mod P], and for six of the eight external
//     rounds (1, 2, 3, 5, 6, 7) the constant is not an instruction at all: the layer is linear, M x + rc' = M (x + c) with
//     c = M^-1 rc', and K = c * 2^32 mod P rides as a 64-bit SCALAR addend on the last product of the S-boxes in front of the
//     layer (it was the literal 0), so that x = REDC(y) (sredc_all: 2 instructions per cell, not 3).  Round 0's constants follow no
//     S-box and round 4's ride in the last internal round, where every addend is taken: those two keep the 64-bit add.
//     The factor 2^-32 is not compensated: the cells of a round share a known
//     representation factor R^e that the (homogeneous) linear layers carry along and the S-box maps to R^(7e-6); the round
//     constants are stored pre-scaled, and only the two layers that must hand back Montgomery form (before the internal
//     rounds, and at the end) multiply by a correction constant (poseidon2_arith.hpp: representation tracking).
// Results are congruent mod P at every step and the words that leave the permutation are canonical, so the output is
// bit-identical to the reduce-everywhere form (5 949 VALU instructions per permutation by PMC, down from ~14.5 k).
//
// Magnitude bounds (rho = P / 2^32 = 0.46875; sredc(t) in [t/2^32 - P/2, t/2^32 + P/2); int32 holds 1.0667 P):
//   redc64s output                     |x| <= 57 + P/2                           (external rounds' S-box input)
//   sbox7s(|x| <= 0.945 P)             |x2| < 0.919 P, |x3| < 0.907 P, |x4| < 0.896 P, |x7| < 0.881 P; products <= 0.893 P^2 < 1.2 P^2
//   ... with a folded constant          |x3 x4 + K| <= 0.907 * 0.896 P^2 + P (K canonical), the output bound grows by at most 1 (B_SBOX_K)
//   m_ext64s(any int32 cells)          rows sum to <= 112, |y| <= 112 * 2^31 < 2^38
//   sredc_all output                   |x| <= 57 + P/2, as redc64s
//   red64ks<MID>/<END> output          |x| < K1 + 26 + P/2  = 0.626 P / 0.555 P    (K1 = R^2801, R^400 mod P)
//   internal rounds                    cell i: sredc(d_i s_i + sum_r [+ rc]) with d_i < P: B -> rho B + P/2 + 2 has its fixed
//                                      point at 0.9412 P, 0.945 P is invariant; |sum| < 22.7 P < 2^37; |sum_r| < 0.791 P thanks to
//                                      the balanced low word of sum.
//   paired internal rounds             (rounds 1..20, poseidon2_arith.hpp: internal_round_pair) constants centred to +-P/2; dot-product
//                                      groups < 2.2 P^2 < 2^63, folded to < 0.14 P^2; |sig1| <= P/2 + 4, |sig2| < 0.57 P; cell operands
//                                      <= 0.73 P^2, cells < 0.85 P
// ---------------------------------------------------------------------------------------------------------------
// Device parameter table (round constants scaled by p2_rc_scale(i) so that they can ride in a REDC accumulator of the
// round's representation): [0,96) external rounds 0-3 | [96,117) internal rounds | [117,213) external rounds 4-7 |
// [216,240) internal diagonal (plain Montgomery form, used as a multiplier; 32-byte aligned) | [240,288) the constants of the
// paired internal rounds derived from it (p2_pair_consts: E[24], A[24], centred, as two's-complement words) | [288,672) the folded
// external constants (p2_fold_consts): eight blocks of 24 pairs {K, 0}, one block per external round's S-boxes in execution order;
// blocks 0, 1, 2 carry rounds 1, 2, 3, blocks 4, 5, 6 rounds 5, 6, 7, and blocks 3 and 7 are zero (the layers behind those S-boxes
// change the representation, red64ks_all), so that each external-round loop keeps one copy of its S-boxes.  Words [0,288) are what
// they were before the region existed: the quad kernels read [0,240) only.  poseidon2_arith.hpp: p2_build_table builds all of it.
// Input: cells < P (canonical; the capacity of a sponge's later blocks: the signed words carried from the permutation before).
// Output: canonical (SIGNED: the carried capacity).
// [LO, HI) is the LIVE RANGE: the output cells the caller reads.  A sponge that absorbs again reads the capacity, <16, 24> (the rate is
// overwritten by the next 16 columns); its last permutation and every Merkle fold read the digest, <0, 8>.  The compiler drops what plain
// C computes for a dead cell by itself, but not the pinned multiply-adds, so the last layer is split: all 24 S-boxes and the layer's blocks
// and column sums are computed as ever (every output needs them), and the final add, the reduction that restores the Montgomery form,
// canon and the store run for the live cells only.  io[] keeps its input words in the dead cells.
typedef uint32_t sgpr8 __attribute__((ext_vector_type(8)));
typedef uint64_t sgpr4q __attribute__((ext_vector_type(4)));  // the same 32 bytes as four 64-bit addends (SGPR pairs)
static_assert(DIAG_OFF % 8 == 0 && PAIR_OFF % 8 == 0 && FOLD_OFF % 8 == 0 && CELLS % 8 == 0, "the tables are read as 32-byte octets");
// Half h (12 cells) of the S-boxes of external round `block` (0..7 in execution order), with the next round's folded constants on the
// last products.  The 12 pairs {K, 0} are fetched like the other tables: the compiler's own 32-byte scalar loads from the wave-uniform
// table pointer, pinned by an empty statement; 24 SGPRs are live, for this half only.
__device__ __forceinline__ void sbox_half_folded(i32* s, const uint32_t* __restrict__ prm, int block, int h) {
    const sgpr4q* fp = reinterpret_cast<const sgpr4q*>(prm + FOLD_OFF + block * P2_FOLD_BLOCK + h * CELLS);
    sgpr4q f0 = fp[0], f1 = fp[1], f2 = fp[2];
    asm volatile("" : "+s"(f0), "+s"(f1), "+s"(f2));
    i64 K[CELLS / 2];
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] = (i64)f0[i], K[4 + i] = (i64)f1[i], K[8 + i] = (i64)f2[i];
    sbox7s_n<CELLS / 2>(s + h * (CELLS / 2), K);
}
// SIGNED (a sponge's non-final permutations, live cells inside the capacity): the live cells leave as the signed words of the last
// reduction (|v| < 0.555 P), without canon; the next permutation bit-casts them back and its first layer accepts any int32.
template <int LO = 0, int HI = CELLS, bool SIGNED = false>
__device__ __forceinline__ void poseidon2_mix(uint32_t* io, const uint32_t* __restrict__ prm) {
    static_assert(!SIGNED || LO >= RATE, "only capacity cells are carried signed");
    i32 s[CELLS];
    i64 y[CELLS];
#pragma unroll
    for (int i = 0; i < CELLS; ++i) s[i] = (i32)io[i];
    // initial external layer; round-0 constants ride in the reduction
    m_ext64s(s, y);
    redc64s_all(y, prm, s);
    // external rounds 0..3: S-box with the NEXT round's folded constants on its last product, layer, bare reduction (after round 3
    // the block is zero and only cell 0 has a constant: the first internal round's)
#pragma unroll 1
    for (int r = 0; r < RF_HALF; ++r) {
        asm volatile("" : "+s"(r));  // the counter stays a scalar (see the second loop)
        sbox_half_folded(s, prm, r, 0);  // two halves: 12 independent chains are enough ILP and halve the live 64-bit temporaries
        sbox_half_folded(s, prm, r, 1);
        m_ext64s(s, y);
        if (r < RF_HALF - 1) {
            sredc_all(y, s);
        } else {  // back to the Montgomery representation for the internal rounds
            red64ks_all<K1_MID, K2_MID, true>(y, prm[96], s);
        }
    }
    // internal rounds: cells[i] = sum + diag[i]*cells[i].  Rounds 1..20 go two at a time (internal_round_pair: cells 1..23 return
    // to 32 bits once per pair); in the last one sum is accumulated in 64 bits, turned into sum_r = sum * 2^32 mod P by one
    // reduction, and rides in each cell's REDC accumulator together with external round 4's constants.
    // The 24 diagonal words are wave-uniform, and the multiply-adds read them as their one scalar operand.  Loaded as plain scalars
    // the compiler re-issues the s_load (+ s_waitcnt stall) in every internal round; held in VGPRs they cost 24 registers.  So each table
    // is fetched ONCE by 32-byte scalar loads from the wave-uniform table pointer straight into SGPR octets, and the octets then pass
    // through an empty volatile statement as SGPR in/out operands: behind it they are values the compiler can neither rematerialise
    // from memory nor widen, the wait is the compiler's own, in front of the statement, and no vector instruction is spent on
    // them (the tables used to come through 18 vector loads and 72 v_readfirstlane).  The loads stay the compiler's, not text
    // inside the statement: a statement that takes the table pointer makes the pointer escape, and every round constant of the
    // kernel then comes through a vector load and a full wait (tools/experiments/README.md).
    // The constants of the paired rounds (E, A: poseidon2_arith.hpp) are fetched in front of the pairs, the diagonal itself only
    // behind them, for the single last round: 48 + a few SGPRs are live in the loop, not 72.
    {
        const sgpr8* kp = reinterpret_cast<const sgpr8*>(prm + PAIR_OFF);
        sgpr8 k0 = kp[0], k1 = kp[1], k2 = kp[2], k3 = kp[3], k4 = kp[4], k5 = kp[5];
        asm volatile("" : "+s"(k0), "+s"(k1), "+s"(k2), "+s"(k3), "+s"(k4), "+s"(k5));
        i32 pk[2 * CELLS];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            pk[i] = (i32)k0[i], pk[8 + i] = (i32)k1[i], pk[16 + i] = (i32)k2[i];
            pk[24 + i] = (i32)k3[i], pk[32 + i] = (i32)k4[i], pk[40 + i] = (i32)k5[i];
        }
#pragma unroll 1
        for (int r = 0; r < RP - 1; r += 2) {
            internal_round_pair(s, pk, pk + CELLS, prm + 97 + r);
        }
    }
    uint32_t diag[CELLS];
    {
        const sgpr8* dp = reinterpret_cast<const sgpr8*>(prm + DIAG_OFF);
        sgpr8 d0 = dp[0], d1 = dp[1], d2 = dp[2];
        asm volatile("" : "+s"(d0), "+s"(d1), "+s"(d2));
#pragma unroll
        for (int i = 0; i < 8; ++i) diag[i] = d0[i], diag[8 + i] = d1[i], diag[16 + i] = d2[i];
    }
    internal_round<true>(s, diag, prm + 117);  // external round 4's constants ride in the last internal round
    // external rounds 4..7: one copy of the S-boxes and of the layer's core for all four rounds; the loop is left from its middle in
    // the last round, whose finish (live cells only) stands behind it
    i64 t[4];
#pragma unroll 1
    for (int r = 0;; ++r) {
        asm volatile("" : "+s"(r));  // the counter stays a scalar: left alone it becomes a 64-bit byte offset in VGPRs, compared and read back per round
        sbox_half_folded(s, prm, RF_HALF + r, 0);  // rounds 5..7's constants; the last round's block is zero
        sbox_half_folded(s, prm, RF_HALF + r, 1);
        m_ext64s_core(s, y, t);
        if (r == RF_HALF - 1) break;
        m_ext64s_finish(y, t);
        sredc_all(y, s);
    }
    m_ext64s_finish<LO, HI>(y, t);
    red64ks_all<K1_END, K2_END, false, LO, HI>(y, 0u, s);
#pragma unroll
    for (int i = LO; i < HI; ++i) io[i] = SIGNED ? (uint32_t)s[i] : canon(s[i]);  // canonical Montgomery words leave the permutation (SIGNED: the carried capacity)
}

// Occupancy: the stage-wise order fixes the register pressure (the statements are volatile), so the stages are 12 cells wide
// (3 four-cell groups in the linear layer): 100-120 VGPRs, four waves per SIMD without spills.  Five (96 VGPRs) spills.
// hash_rows: lane = row.  matrix is column-major rows x cols.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void hash_rows_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ matrix,
                                                        const uint32_t* __restrict__ prm, uint32_t rows, uint32_t cols) {
    uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    uint32_t s[CELLS];
#pragma unroll
    for (int i = 0; i < CELLS; ++i) s[i] = 0u;
    const uint32_t* p = matrix + r;
    // Two inlined permutations: the loop takes every block of 16 columns but the last and hands on the capacity only (cells 16..23:
    // the rate is overwritten by the next block); the peeled one is the last block, full (cols a multiple of 16), padded with zeros, or
    // empty (cols == 0: the digest of the zero state), and hands on the digest only.
    uint32_t c = 0;
    for (; c + RATE < cols; c += RATE) {
#pragma unroll
        for (int i = 0; i < RATE; ++i) s[i] = p[(size_t)(c + i) * rows];
        poseidon2_mix<RATE, CELLS, true>(s, prm);  // the capacity is carried as signed words: nothing but the next permutation reads it
    }
#pragma unroll
    for (int i = 0; i < RATE; ++i) s[i] = (c + i < cols) ? p[(size_t)(c + i) * rows] : 0u;
    poseidon2_mix<0, 8>(s, prm);
    uint4* o = reinterpret_cast<uint4*>(out + (size_t)r * 8);
    o[0] = make_uint4(s[0], s[1], s[2], s[3]);
    o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// hash_fold: lane = output node; io[out+i] = H(io[in+2i] || io[in+2i+1]).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void hash_fold_kernel(uint32_t* __restrict__ io, const uint32_t* __restrict__ prm,
                                                        uint32_t input_size, uint32_t output_size) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= output_size) return;
    const uint4* src = reinterpret_cast<const uint4*>(io + ((size_t)input_size + 2 * (size_t)i) * 8);
    uint32_t s[CELLS];
    uint4 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3];
    s[0] = v0.x; s[1] = v0.y; s[2] = v0.z; s[3] = v0.w;
    s[4] = v1.x; s[5] = v1.y; s[6] = v1.z; s[7] = v1.w;
    s[8] = v2.x; s[9] = v2.y; s[10] = v2.z; s[11] = v2.w;
    s[12] = v3.x; s[13] = v3.y; s[14] = v3.z; s[15] = v3.w;
#pragma unroll
    for (int k = 16; k < CELLS; ++k) s[k] = 0u;
    poseidon2_mix<0, 8>(s, prm);
    uint4* o = reinterpret_cast<uint4*>(io + ((size_t)output_size + i) * 8);
    o[0] = make_uint4(s[0], s[1], s[2], s[3]);
    o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// hash_fold with an indirection: out[j] = H(in[sel[2j]] || in[sel[2j+1]]).  The levels of a SPARSE Merkle tree (the zkVM
// memory image, bx_image.h: 2^22 leaves of which a few hundred exist) are folded with it: the host lists, per level, which
// two digests of the level below (or that level's all-zero digest) feed each surviving parent.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void hash_fold_indexed_kernel(uint32_t* out, const uint32_t* in,  // (bx_hash_fold_indexed refuses an out that overlaps in)
                                                                const uint32_t* __restrict__ sel, const uint32_t* __restrict__ prm,
                                                                uint32_t count, uint32_t n_in) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    uint2 pr = reinterpret_cast<const uint2*>(sel)[j];
    pr.x = pr.x < n_in ? pr.x : n_in - 1;  // sel comes from the caller: an entry beyond the pool must not become an out-of-bounds read
    pr.y = pr.y < n_in ? pr.y : n_in - 1;
    const uint4* a = reinterpret_cast<const uint4*>(in + (size_t)pr.x * 8);
    const uint4* b = reinterpret_cast<const uint4*>(in + (size_t)pr.y * 8);
    uint32_t s[CELLS];
    uint4 v0 = a[0], v1 = a[1], v2 = b[0], v3 = b[1];
    s[0] = v0.x; s[1] = v0.y; s[2] = v0.z; s[3] = v0.w;
    s[4] = v1.x; s[5] = v1.y; s[6] = v1.z; s[7] = v1.w;
    s[8] = v2.x; s[9] = v2.y; s[10] = v2.z; s[11] = v2.w;
    s[12] = v3.x; s[13] = v3.y; s[14] = v3.z; s[15] = v3.w;
#pragma unroll
    for (int k = 16; k < CELLS; ++k) s[k] = 0u;
    poseidon2_mix<0, 8>(s, prm);
    uint4* o = reinterpret_cast<uint4*>(out + (size_t)j * 8);
    o[0] = make_uint4(s[0], s[1], s[2], s[3]);
    o[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// Several levels of a LARGE layer in one launch, every lane busy: lane j folds the 2^L consecutive input digests
// [2^L j, 2^L (j+1)) depth first — at most L digests are alive while the next pair is hashed — and writes every intermediate
// node to its place in the tree.  2^L - 1 permutations per lane, so the lane efficiency is that of the per-layer kernel, but a
// 2^22-leaf tree needs two launches down to the 2^17-node layer where the latency-bound kernel takes over instead of five, and
// the intermediate layers are never read back.
__device__ __forceinline__ void fold_pair(uint32_t* out8, const uint32_t* a8, const uint32_t* b8, const uint32_t* __restrict__ prm) {
    uint32_t s[CELLS];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = a8[k], s[8 + k] = b8[k];
#pragma unroll
    for (int k = 16; k < CELLS; ++k) s[k] = 0u;
    // Every permutation of a subtree fetches its constants at an offset of its own: sharing one address, the compiler keeps the first
    // permutation's round constants in SGPRs for the later ones and, with the paired rounds' 48 words beside them, spills.
    // (a scalar zero the compiler cannot see through, added to the pointer: the loads stay scalar loads of the same table)
    uint32_t z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    poseidon2_mix<0, 8>(s, prm + z);
#pragma unroll
    for (int k = 0; k < 8; ++k) out8[k] = s[k];
}
__device__ __forceinline__ void ld_digest(uint32_t* d, const uint32_t* p) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}
__device__ __forceinline__ void st_digest(uint32_t* p, const uint32_t* d) {
    reinterpret_cast<uint4*>(p)[0] = make_uint4(d[0], d[1], d[2], d[3]);
    reinterpret_cast<uint4*>(p)[1] = make_uint4(d[4], d[5], d[6], d[7]);
}
// node `idx` of the layer `lvl` levels above the input layer (lvl = 1: parents of inputs), computed depth first
template <int LVL>
__device__ __forceinline__ void fold_subtree(uint32_t* out8, uint32_t* __restrict__ io, const uint32_t* __restrict__ prm, size_t input_size, size_t idx) {
    uint32_t a[8], b[8];
    if constexpr (LVL == 1) {
        ld_digest(a, io + (input_size + 2 * idx) * 8);
        ld_digest(b, io + (input_size + 2 * idx + 1) * 8);
    } else {
        fold_subtree<LVL - 1>(a, io, prm, input_size, 2 * idx);
        fold_subtree<LVL - 1>(b, io, prm, input_size, 2 * idx + 1);
    }
    fold_pair(out8, a, b, prm);
    st_digest(io + ((input_size >> LVL) + idx) * 8, out8);
}
template <int L>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void hash_fold_deep_kernel(uint32_t* __restrict__ io, const uint32_t* __restrict__ prm,
                                                                                               uint32_t input_size) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (input_size >> L)) return;
    uint32_t top[8];
    fold_subtree<L>(top, io, prm, input_size, j);
}

// Small layers in one launch: a workgroup owns `per_wg` (<= 512) consecutive input digests and folds them `levels`
// levels deep through LDS, writing every intermediate layer.  Used once a layer no longer fills the chip, where each
// separate launch would cost a full single-wave permutation latency.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void hash_fold_multi_kernel(uint32_t* __restrict__ io, const uint32_t* __restrict__ prm,
                                                              uint32_t input_size, uint32_t per_wg, int levels) {
    __shared__ uint32_t sh[256 * 8];
    const uint32_t tid = threadIdx.x;
    uint32_t width = per_wg >> 1;  // outputs of this workgroup at the current level
    uint32_t out_size = input_size >> 1;
    uint32_t s[CELLS];
    if (tid < width) {
        const uint32_t i = blockIdx.x * width + tid;
        const uint4* src = reinterpret_cast<const uint4*>(io + ((size_t)input_size + 2 * (size_t)i) * 8);
        uint4 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3];
        s[0] = v0.x; s[1] = v0.y; s[2] = v0.z; s[3] = v0.w;
        s[4] = v1.x; s[5] = v1.y; s[6] = v1.z; s[7] = v1.w;
        s[8] = v2.x; s[9] = v2.y; s[10] = v2.z; s[11] = v2.w;
        s[12] = v3.x; s[13] = v3.y; s[14] = v3.z; s[15] = v3.w;
#pragma unroll
        for (int k = 16; k < CELLS; ++k) s[k] = 0u;
        poseidon2_mix<0, 8>(s, prm);
        uint4* o = reinterpret_cast<uint4*>(io + ((size_t)out_size + i) * 8);
        o[0] = make_uint4(s[0], s[1], s[2], s[3]);
        o[1] = make_uint4(s[4], s[5], s[6], s[7]);
    }
    for (int lvl = 1; lvl < levels; ++lvl) {
        if (tid < width) {
#pragma unroll
            for (int k = 0; k < 8; ++k) sh[tid * 8 + k] = s[k];
        }
        __syncthreads();
        width >>= 1;
        out_size >>= 1;
        if (tid < width) {
#pragma unroll
            for (int k = 0; k < 16; ++k) s[k] = sh[tid * 16 + k];
#pragma unroll
            for (int k = 16; k < CELLS; ++k) s[k] = 0u;
            poseidon2_mix<0, 8>(s, prm);
            uint4* o = reinterpret_cast<uint4*>(io + ((size_t)out_size + blockIdx.x * width + tid) * 8);
            o[0] = make_uint4(s[0], s[1], s[2], s[3]);
            o[1] = make_uint4(s[4], s[5], s[6], s[7]);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The same permutation spread over a QUAD of lanes, for the layers that no longer fill the chip.  There the cost of a level
// is the latency of one permutation on one lane (6.6 k dependent-ish instructions, ~12 us), not throughput; four lanes per
// permutation cut the per-lane instruction stream to ~2.3 k.  Lane q of a quad holds cells 4k + q (slot k = 0..5):
//   * an external layer's M4 block k is the slot-k values of the four lanes: each lane computes its own row of M4 from the
//     three other lanes' values (v_mov_b32_dpp quad_perm rotations) with per-lane coefficients; the column sums T_j are lane-local;
//   * the S-boxes and the returns to 32 bits are per cell and reuse the stage-wise helpers at width 6;
//   * an internal round sums six cells per lane and all-reduces the 64-bit partial sums over the quad with two DPP steps;
//     every lane runs the S-box of its slot 0 and only lane 0 (cell 0) keeps it.
// Per-lane round constants and diagonal entries come from a copy of the parameter table in LDS.  The arithmetic per cell is
// exactly poseidon2_mix's (same representation tracking, same bounds), so the words that leave are the same words.
constexpr int QS = CELLS / 4;  // slots per lane
__device__ __forceinline__ i32 quad_rot1(i32 v) { return __builtin_amdgcn_update_dpp(0, v, 0x39, 0xf, 0xf, false); }  // from lane (q+1)&3
__device__ __forceinline__ i32 quad_rot2(i32 v) { return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false); }  // (q+2)&3
__device__ __forceinline__ i32 quad_rot3(i32 v) { return __builtin_amdgcn_update_dpp(0, v, 0x93, 0xf, 0xf, false); }  // (q+3)&3
__device__ __forceinline__ i32 quad_xor1(i32 v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false); }
__device__ __forceinline__ i64 add_u32v(i64 c, uint32_t k, int alt) {  // c + k, k a per-lane unsigned word
#if defined(__HIP_DEVICE_COMPILE__)
    i64 r;
    BX_MAD_ASM("v_mad_u64_u32", "%1, 1, %2", "v"(k), "v"(c));
    return r;
#else
    (void)alt;
    return c + (i64)k;
#endif
}
struct QuadCoef {
    i32 c0, c1, c3;  // this lane's row of M4 = [[5,7,1,3],[4,6,1,1],[1,3,5,7],[1,1,4,6]], rotated to start at its own column (c2 = 1)
};
__device__ __forceinline__ void m_ext_quad(const i32* s, i64* y, const QuadCoef& m) {
    i64 t = 0;
#pragma unroll
    for (int k = 0; k < QS; ++k) {
        const i32 x1 = quad_rot1(s[k]), x2 = quad_rot2(s[k]), x3 = quad_rot3(s[k]);
        i64 w = smul(s[k], m.c0, k);
        w = smad(x1, m.c1, w, k + 1);
        w = smadc<1>(x2, w, k + 2);
        w = smad(x3, m.c3, w, k + 3);
        y[k] = w;
        t += w;
    }
#pragma unroll
    for (int k = 0; k < QS; ++k) y[k] += t;
}
__device__ __forceinline__ void redc_quad(const i64* y, const uint32_t* __restrict__ rc /* LDS, this lane's entries 4k apart */, i32* s) {
    i64 acc[QS];
#pragma unroll
    for (int k = 0; k < QS; ++k) acc[k] = add_u32v(y[k], rc[4 * k], k);
    sredc_n<QS>(acc, s);
}
template <uint32_t K1, uint32_t K2>
__device__ __forceinline__ void redk_quad(const i64* y, uint32_t add0 /* this lane's addend for slot 0 (0 = none) */, i32* s) {
    i64 acc[QS];
#pragma unroll
    for (int k = 0; k < QS; ++k) acc[k] = umul_k((uint32_t)y[k], K1, k);
    acc[0] = add_u32v(acc[0], add0, 0);
#pragma unroll
    for (int k = 0; k < QS; ++k) acc[k] = smad_k((i32)(y[k] >> 32), K2, acc[k], k + 1);
    sredc_n<QS>(acc, s);
}
template <bool RC_ALL>
__device__ __forceinline__ void internal_round_quad(i32* s, const i32* diag, uint32_t rc0 /* lane 0: the round's constant, else 0 */,
                                                    const uint32_t* __restrict__ rc_all, uint32_t keep_mask) {
    const i32 sb = sbox7s(s[0]);
    s[0] = (i32)(((uint32_t)sb & keep_mask) | ((uint32_t)s[0] & ~keep_mask));  // only cell 0 has an S-box in these rounds
    i64 pa = smulc<1>(s[0], 0);
#pragma unroll
    for (int k = 1; k < QS; ++k) pa = smadc<1>(s[k], pa, k);
    {  // all-reduce over the quad
        i64 o = (i64)(((uint64_t)(uint32_t)quad_xor1((i32)(pa >> 32)) << 32) | (uint32_t)quad_xor1((i32)(uint32_t)pa));
        pa += o;
        o = (i64)(((uint64_t)(uint32_t)quad_rot2((i32)(pa >> 32)) << 32) | (uint32_t)quad_rot2((i32)(uint32_t)pa));
        pa += o;
    }
    const i64 c = smulc<1>(internal_sum_rs(pa), 1);
    i64 tt[QS];
#pragma unroll
    for (int k = 0; k < QS; ++k) {
        if (RC_ALL) tt[k] = smad(s[k], diag[k], add_u32v(c, rc_all[4 * k], 2 * k), 2 * k + 1);
        else if (k == 0) tt[k] = smad(s[k], diag[k], add_u32v(c, rc0, 0), 1);
        else tt[k] = smad(s[k], diag[k], c, k + 1);
    }
    sredc_n<QS>(tt, s);
}
// in: this lane's cells (canonical); out: this lane's cells (canonical).  shp = the parameter table in LDS.
__device__ __forceinline__ void poseidon2_mix_quad(uint32_t* io, const uint32_t* __restrict__ shp, uint32_t q) {
    i32 s[QS];
    i64 y[QS];
    const bool odd = q & 1;
    const QuadCoef m{odd ? 6 : 5, odd ? 1 : 7, odd ? 4 : 3};
    const uint32_t keep = q == 0 ? 0xffffffffu : 0u;
#pragma unroll
    for (int k = 0; k < QS; ++k) s[k] = (i32)io[k];
    m_ext_quad(s, y, m);
    redc_quad(y, shp + q, s);
#pragma unroll 1
    for (int r = 0; r < RF_HALF; ++r) {
        sbox7s_n<QS>(s);
        m_ext_quad(s, y, m);
        if (r < RF_HALF - 1) redc_quad(y, shp + (r + 1) * CELLS + q, s);
        else redk_quad<K1_MID, K2_MID>(y, shp[96] & keep, s);
    }
    i32 diag[QS];
#pragma unroll
    for (int k = 0; k < QS; ++k) diag[k] = (i32)shp[DIAG_OFF + 4 * k + q];
#pragma unroll 1
    for (int r = 0; r < RP - 1; ++r) internal_round_quad<false>(s, diag, shp[97 + r] & keep, nullptr, keep);
    internal_round_quad<true>(s, diag, 0u, shp + 117 + q, keep);
#pragma unroll 1
    for (int r = 0; r < RF_HALF; ++r) {
        sbox7s_n<QS>(s);
        m_ext_quad(s, y, m);
        if (r < RF_HALF - 1) redc_quad(y, shp + 117 + (r + 1) * CELLS + q, s);
        else redk_quad<K1_END, K2_END>(y, 0u, s);
    }
#pragma unroll
    for (int k = 0; k < QS; ++k) io[k] = canon(s[k]);
}

// Small Merkle layers, four lanes per node: a workgroup owns `per_wg` (<= 512) consecutive input digests and folds them
// `levels` levels deep through LDS, writing every intermediate layer (as hash_fold_multi_kernel does with one lane per node).
__global__ __launch_bounds__(1024) void hash_fold_quad_kernel(uint32_t* __restrict__ io, const uint32_t* __restrict__ prm, uint32_t input_size,
                                                              uint32_t per_wg, int levels) {
    __shared__ uint32_t sh[256 * 8];
    __shared__ uint32_t shp[DIAG_OFF + 24];
    const uint32_t tid = threadIdx.x, q = tid & 3, node = tid >> 2;
    for (uint32_t i = tid; i < DIAG_OFF + 24; i += blockDim.x) shp[i] = prm[i];
    uint32_t width = per_wg >> 1;  // nodes this workgroup produces at the current level
    uint32_t out_size = input_size >> 1;
    for (int lvl = 0; lvl < levels; ++lvl) {
        const bool active = node < width;
        uint32_t s[QS];
        if (active) {
            if (lvl == 0) {
                const uint32_t* src = io + ((size_t)input_size + 2 * ((size_t)blockIdx.x * width + node)) * 8;
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = src[4 * k + q];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = sh[node * 16 + 4 * k + q];
            }
            s[4] = 0u;
            s[5] = 0u;
        }
        __syncthreads();  // the level's inputs are in registers (and, at level 0, the parameter table is in LDS)
        if (active) {
            poseidon2_mix_quad(s, shp, q);
            uint32_t* o = io + ((size_t)out_size + (size_t)blockIdx.x * width + node) * 8;
            o[q] = s[0];
            o[4 + q] = s[1];
            sh[node * 8 + q] = s[0];
            sh[node * 8 + 4 + q] = s[1];
        }
        __syncthreads();
        width >>= 1;
        out_size >>= 1;
    }
}

// One step of the Fiat-Shamir transcript on the device (transcript.hpp's Transcript::commit / random_elem, i.e. risc0_zkp's
// Poseidon2Rng): four lanes hold the 24 cells as poseidon2_mix_quad wants them (lane q: cells 4k + q).  A step is 1-2 sequential
// permutations (8.7 us each on a quad) against ~150 us for the host round trip it replaces; the long sponges of the transcript
// (coeff_u, the final coefficients) stay on the host, where a permutation takes ~1 us.
__global__ __launch_bounds__(64) void transcript_step_kernel(uint32_t* __restrict__ state, const uint32_t* __restrict__ digests, uint32_t n_commit,
                                                            uint32_t* __restrict__ out, uint32_t n_elems, const uint32_t* __restrict__ prm) {
    __shared__ uint32_t shp[DIAG_OFF + 24];
    const uint32_t tid = threadIdx.x, q = tid & 3;
    for (uint32_t i = tid; i < DIAG_OFF + 24; i += blockDim.x) shp[i] = prm[i];
    __syncthreads();
    if (tid >= 4) return;
    uint32_t s[QS];
#pragma unroll
    for (int k = 0; k < QS; ++k) s[k] = state[4 * k + q];
    uint32_t pool = state[24];
    for (uint32_t i = 0; i < n_commit; ++i) {
        if (pool != 0) {  // elements were handed out since the last permutation: the pool is discarded first
            poseidon2_mix_quad(s, shp, q);
            pool = 0;
        }
        s[0] = fp_add(s[0], digests[8 * i + q]);
        s[1] = fp_add(s[1], digests[8 * i + 4 + q]);
        poseidon2_mix_quad(s, shp, q);
    }
    for (uint32_t e = 0; e < n_elems; ++e) {
        if (pool == 16) {
            poseidon2_mix_quad(s, shp, q);
            pool = 0;
        }
        const uint32_t slot = pool >> 2;
        const uint32_t v = slot == 0 ? s[0] : slot == 1 ? s[1] : slot == 2 ? s[2] : s[3];
        if ((pool & 3u) == q) out[e] = v;
        ++pool;
    }
#pragma unroll
    for (int k = 0; k < QS; ++k) state[4 * k + q] = s[k];
    if (q == 0) state[24] = pool;
}

const char* poseidon2_upload_params(bx_ctx* c) {
    uint32_t h[P2_TABLE];
    // poseidon2_arith.hpp: the scaled round constants, the diagonal, the paired rounds' constants and the folded external constants,
    // which are checked against the layer (M c == rc') as they are derived
    if (!p2_build_table(c->h_rc, c->h_diag, h)) return "poseidon2_upload_params: the folded round constants do not reproduce the stored ones";
    if (!c->d_p2) BX_HIP(c, hipMalloc(&c->d_p2, sizeof h));
    BX_HIP(c, hipMemcpyAsync(c->d_p2, h, sizeof h, hipMemcpyHostToDevice, c->stream));
    BX_HIP(c, stream_wait(c));
    return nullptr;
}

static const char* launch_hash_rows(bx_ctx* c, uint32_t* out, const uint32_t* matrix, size_t rows, size_t cols) {
    if (rows == 0) return nullptr;
    unsigned bs = (unsigned)c->hash_rows_block;
    hipLaunchKernelGGL(hash_rows_kernel, dim3((unsigned)((rows + bs - 1) / bs)), dim3(bs), 0, c->stream, out, matrix, c->d_p2,
                       (uint32_t)rows, (uint32_t)cols);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
static const char* launch_hash_fold(bx_ctx* c, uint32_t* io, size_t input_size, size_t output_size) {
    if (output_size == 0) return nullptr;
    hipLaunchKernelGGL(hash_fold_kernel, dim3((unsigned)((output_size + 255) / 256)), dim3(256), 0, c->stream, io, c->d_p2,
                       (uint32_t)input_size, (uint32_t)output_size);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
template <int L>
static const char* launch_hash_fold_deep(bx_ctx* c, uint32_t* io, size_t size) {
    hipLaunchKernelGGL(hash_fold_deep_kernel<L>, dim3((unsigned)(((size >> L) + 255) / 256)), dim3(256), 0, c->stream, io, c->d_p2, (uint32_t)size);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
// small layers: four lanes per node (fold_quad, the default) or one
static const char* launch_hash_fold_small(bx_ctx* c, uint32_t* io, size_t size, size_t per_wg, int levels) {
    if (c->fold_quad)
        hipLaunchKernelGGL(hash_fold_quad_kernel, dim3((unsigned)(size / per_wg)), dim3((unsigned)(2 * per_wg)), 0, c->stream, io, c->d_p2,
                           (uint32_t)size, (uint32_t)per_wg, levels);
    else
        hipLaunchKernelGGL(hash_fold_multi_kernel, dim3((unsigned)(size / per_wg)), dim3(256), 0, c->stream, io, c->d_p2, (uint32_t)size,
                           (uint32_t)per_wg, levels);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
HashLaunchers poseidon2_launchers() { return {launch_hash_rows, launch_hash_fold, launch_hash_fold_deep<3>, launch_hash_fold_deep<2>, launch_hash_fold_small}; }

}  // namespace bx

using namespace bx;

extern "C" const char* bx_poseidon2_set_params(bx_ctx* c, const uint32_t* rc213, const uint32_t* diag24) try {
    if (!c) return "bx_poseidon2_set_params: null ctx";
    BX_REQUIRE(c, rc213 && diag24, "poseidon2_set_params: null table");
    // a prover snapshots the table for its host transcript at create time and bx_verify_segment uses the compiled-in one:
    // changing the device table under a live prover would make its trees and its transcript disagree
    BX_REQUIRE(c, c->live_provers == 0, "poseidon2_set_params: destroy the provers of this ctx first (their transcripts hold the old table)");
    BX_ENTER(c);
    for (int i = 0; i < 213; ++i) c->h_rc[i] = rc213[i] % P;
    for (int i = 0; i < 24; ++i) c->h_diag[i] = diag24[i] % P;
    return poseidon2_upload_params(c);
} BX_ABI_CATCH(c, "bx_poseidon2_set_params")
extern "C" const char* bx_poseidon2_get_params(bx_ctx* c, uint32_t* rc213, uint32_t* diag24) try {
    if (!c) return "bx_poseidon2_get_params: null ctx";
    for (int i = 0; i < 213; ++i) rc213[i] = c->h_rc[i];
    for (int i = 0; i < 24; ++i) diag24[i] = c->h_diag[i];
    return nullptr;
} BX_ABI_CATCH(c, "bx_poseidon2_get_params")

extern "C" const char* bx_hash_fold_indexed(bx_ctx* c, bx_buf out, bx_buf in, bx_buf sel, size_t count) try {
    if (!c) return "bx_hash_fold_indexed: null ctx";
    BX_REQUIRE(c, count <= out.len / 8 && count <= sel.len / 2, "hash_fold_indexed: out or sel too small");
    BX_REQUIRE(c, count <= 0xffffffffu && in.len / 8 <= 0xffffffffu, "hash_fold_indexed: too many digests");
    if (count == 0) return nullptr;
    BX_REQUIRE(c, out.dptr && in.dptr && sel.dptr && in.len >= 8, "hash_fold_indexed: null or empty buffer");
    BX_REQUIRE(c, !bufs_overlap(out, in), "hash_fold_indexed: out and in overlap");
    BX_REQUIRE(c, !bufs_overlap(out, sel), "hash_fold_indexed: out and sel overlap");
    BX_ENTER(c);
    OpScope op(c, "hash_fold_indexed", 104.0 * (double)count);
    hipLaunchKernelGGL(hash_fold_indexed_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, (uint32_t*)out.dptr,
                       (const uint32_t*)in.dptr, (const uint32_t*)sel.dptr, c->d_p2, (uint32_t)count, (uint32_t)(in.len / 8));
    BX_LAUNCH_CHECK(c);
    return nullptr;
} BX_ABI_CATCH(c, "bx_hash_fold_indexed")

extern "C" const char* bx_transcript_step(bx_ctx* c, bx_buf state, bx_buf digests, size_t n_commit, bx_buf out_ext, size_t n_ext) try {
    if (!c) return "bx_transcript_step: null ctx";
    // (no dispatch: the only device-side RNG is Poseidon2's)
    BX_REQUIRE(c, c->hash_suite == SUITE_POSEIDON2, "transcript_step: the device transcript is Poseidon2's (a sha-256 ctx draws on the host)");
    BX_REQUIRE(c, state.dptr != nullptr && state.len >= 25, "transcript_step: the state is 24 cells and the pool counter");
    BX_REQUIRE(c, n_commit <= 64 && n_ext <= 64, "transcript_step: at most 64 commits and 64 challenges per step");
    BX_REQUIRE(c, digests.len >= 8 * n_commit && out_ext.len >= 4 * n_ext, "transcript_step: digests / out too small");
    BX_REQUIRE(c, !bufs_overlap(out_ext, state), "transcript_step: out_ext and state overlap");
    BX_REQUIRE(c, !bufs_overlap(out_ext, digests), "transcript_step: out_ext and digests overlap");
    BX_ENTER(c);
    if (!n_commit && !n_ext) return nullptr;
    OpScope op(c, "transcript_step", 4.0 * (double)(50 + 8 * n_commit + 4 * n_ext));
    hipLaunchKernelGGL(transcript_step_kernel, dim3(1), dim3(64), 0, c->stream, (uint32_t*)state.dptr, (const uint32_t*)digests.dptr, (uint32_t)n_commit,
                       (uint32_t*)out_ext.dptr, (uint32_t)(4 * n_ext), c->d_p2);
    BX_LAUNCH_CHECK(c);
    return nullptr;
} BX_ABI_CATCH(c, "bx_transcript_step")
