// sha256.hip — the `sha-256` hash suite's Merkle hashing for gfx950: the kernels behind Hal::{hash_rows, hash_fold} and the Merkle layers
// on a ctx switched with bx_set_hash_suite, and their launcher table (ctx.hpp: HashLaunchers; entry points and schedule: hal.hip).
//
// Restates risc0_zkp's Sha256 HAL kernels `sha_rows` / `sha_fold` with the conventions of sha256_suite.hpp [EXT: risc0-zkp 3.0.3
// core/hash/sha, recalled].  A compression is pure 32-bit VALU work — 64 rounds of alignbit rotates, bfi Ch / Maj and add3 / xor3
// sums plus the rolling 16-word message schedule — with no memory traffic but its 64-byte block, so the kernels are organised like
// the Poseidon2 ones (poseidon2.hip): one row or one output node per lane, the state and the schedule in VGPRs, round constants
// as literals.  No LDS except in the fused small-layer kernel; the row and fold kernels run at full occupancy.
#include "ctx.hpp"
#include "sha256_suite.hpp"

namespace bx {

__device__ __forceinline__ void sha_init(uint32_t* st) {
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = sha256_iv(i);
}
__device__ __forceinline__ void sha_store(uint32_t* o, const uint32_t* st) {  // digest words: the output bytes as little-endian words
    reinterpret_cast<uint4*>(o)[0] = make_uint4(sha_bswap(st[0]), sha_bswap(st[1]), sha_bswap(st[2]), sha_bswap(st[3]));
    reinterpret_cast<uint4*>(o)[1] = make_uint4(sha_bswap(st[4]), sha_bswap(st[5]), sha_bswap(st[6]), sha_bswap(st[7]));
}
// two digests (a || b) as the 16 big-endian message words of one block
__device__ __forceinline__ void sha_pair_block(uint32_t* w, const uint32_t* a, const uint32_t* b) {
    const uint4 a0 = reinterpret_cast<const uint4*>(a)[0], a1 = reinterpret_cast<const uint4*>(a)[1];
    const uint4 b0 = reinterpret_cast<const uint4*>(b)[0], b1 = reinterpret_cast<const uint4*>(b)[1];
    w[0] = sha_bswap(a0.x), w[1] = sha_bswap(a0.y), w[2] = sha_bswap(a0.z), w[3] = sha_bswap(a0.w);
    w[4] = sha_bswap(a1.x), w[5] = sha_bswap(a1.y), w[6] = sha_bswap(a1.z), w[7] = sha_bswap(a1.w);
    w[8] = sha_bswap(b0.x), w[9] = sha_bswap(b0.y), w[10] = sha_bswap(b0.z), w[11] = sha_bswap(b0.w);
    w[12] = sha_bswap(b1.x), w[13] = sha_bswap(b1.y), w[14] = sha_bswap(b1.z), w[15] = sha_bswap(b1.w);
}
// pair hash from registers: out = compress(IV, a || b), all three as big-endian state words (the tree's inner levels never
// leave registers in the depth-first kernel; only what is stored is byte-swapped)
__device__ __forceinline__ void sha_pair_regs(uint32_t* out, const uint32_t* a, const uint32_t* b) {
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = a[k], w[8 + k] = b[k];
    sha_init(out);
    sha256_compress(out, w);
}

// sha_rows: lane = row of the column-major rows x cols matrix; 16 columns per block, so a wave instruction reads 256 contiguous
// bytes (lane r reads matrix[c * rows + r]).  Full blocks take the fast path; the last one or two blocks (the remaining columns,
// the 0x80 byte and the bit length) are built in registers.
__global__ __launch_bounds__(256) void sha256_rows_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ matrix, uint32_t rows,
                                                          uint32_t cols) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const uint32_t* p = matrix + r;
    uint32_t st[8], w[16];
    sha_init(st);
    uint32_t c = 0;
    for (; c + 16 <= cols; c += 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = p[(size_t)(c + i) * rows];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = sha_elem_word(w[i]);
        sha256_compress(st, w);
    }
    const uint32_t rem = cols - c, nb = rem <= 13 ? 1u : 2u;
    const uint64_t bits = (uint64_t)cols * 32u;
#pragma unroll 1
    for (uint32_t blk = 0; blk < nb; ++blk) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t idx = 16u * blk + (uint32_t)i;
            w[i] = idx < rem ? sha_elem_word(p[(size_t)(c + idx) * rows]) : idx == rem ? 0x80000000u : 0u;
        }
        if (blk + 1 == nb) {
            w[14] = (uint32_t)(bits >> 32);
            w[15] = (uint32_t)bits;
        }
        sha256_compress(st, w);
    }
    sha_store(out + (size_t)r * 8, st);
}

// sha_fold: lane = output node; io[out + i] = pair(io[in + 2i], io[in + 2i + 1]) — two 16-byte loads per digest, one compression.
__global__ __launch_bounds__(256) void sha256_fold_kernel(uint32_t* __restrict__ io, uint32_t input_size, uint32_t output_size) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= output_size) return;
    const uint32_t* src = io + ((size_t)input_size + 2 * (size_t)i) * 8;
    uint32_t st[8], w[16];
    sha_pair_block(w, src, src + 8);
    sha_init(st);
    sha256_compress(st, w);
    sha_store(io + ((size_t)output_size + i) * 8, st);
}

// Several levels of a large layer per launch (as hash_fold_deep_kernel): lane j folds inputs [2^L j, 2^L (j + 1)) depth first and
// writes every intermediate node.
template <int LVL>
__device__ __forceinline__ void sha_fold_subtree(uint32_t* be8, uint32_t* __restrict__ io, size_t input_size, size_t idx) {
    if constexpr (LVL == 1) {
        uint32_t w[16];
        sha_pair_block(w, io + (input_size + 2 * idx) * 8, io + (input_size + 2 * idx + 1) * 8);
        sha_init(be8);
        sha256_compress(be8, w);
    } else {
        uint32_t a[8], b[8];
        sha_fold_subtree<LVL - 1>(a, io, input_size, 2 * idx);
        sha_fold_subtree<LVL - 1>(b, io, input_size, 2 * idx + 1);
        sha_pair_regs(be8, a, b);
    }
    sha_store(io + ((input_size >> LVL) + idx) * 8, be8);
}
template <int L>
__global__ __launch_bounds__(256) void sha256_fold_deep_kernel(uint32_t* __restrict__ io, uint32_t input_size) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (input_size >> L)) return;
    uint32_t top[8];
    sha_fold_subtree<L>(top, io, input_size, j);
}

// Small layers in one launch (as hash_fold_multi_kernel): a workgroup owns `per_wg` (<= 512) consecutive input digests and folds
// them `levels` levels deep, the level between two steps in LDS (as big-endian state words), writing every intermediate layer.
__global__ __launch_bounds__(256) void sha256_fold_multi_kernel(uint32_t* __restrict__ io, uint32_t input_size, uint32_t per_wg, int levels) {
    __shared__ uint32_t sh[256 * 8];
    const uint32_t tid = threadIdx.x;
    uint32_t width = per_wg >> 1;  // outputs of this workgroup at the current level
    uint32_t out_size = input_size >> 1;
    uint32_t st[8];
    if (tid < width) {
        const uint32_t i = blockIdx.x * width + tid;
        const uint32_t* src = io + ((size_t)input_size + 2 * (size_t)i) * 8;
        uint32_t w[16];
        sha_pair_block(w, src, src + 8);
        sha_init(st);
        sha256_compress(st, w);
        sha_store(io + ((size_t)out_size + i) * 8, st);
    }
    for (int lvl = 1; lvl < levels; ++lvl) {
        if (tid < width) {
#pragma unroll
            for (int k = 0; k < 8; ++k) sh[tid * 8 + k] = st[k];
        }
        __syncthreads();
        width >>= 1;
        out_size >>= 1;
        if (tid < width) {
            uint32_t w[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k] = sh[tid * 16 + k];
            sha_init(st);
            sha256_compress(st, w);
            sha_store(io + ((size_t)out_size + blockIdx.x * width + tid) * 8, st);
        }
        __syncthreads();
    }
}

static const char* sha256_rows(bx_ctx* c, uint32_t* out, const uint32_t* matrix, size_t rows, size_t cols) {
    if (rows == 0) return nullptr;
    hipLaunchKernelGGL(sha256_rows_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c->stream, out, matrix, (uint32_t)rows, (uint32_t)cols);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
static const char* sha256_fold(bx_ctx* c, uint32_t* io, size_t input_size, size_t output_size) {
    if (output_size == 0) return nullptr;
    hipLaunchKernelGGL(sha256_fold_kernel, dim3((unsigned)((output_size + 255) / 256)), dim3(256), 0, c->stream, io, (uint32_t)input_size, (uint32_t)output_size);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
template <int L>
static const char* sha256_fold_deep(bx_ctx* c, uint32_t* io, size_t size) {
    hipLaunchKernelGGL(sha256_fold_deep_kernel<L>, dim3((unsigned)(((size >> L) + 255) / 256)), dim3(256), 0, c->stream, io, (uint32_t)size);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
static const char* sha256_fold_small(bx_ctx* c, uint32_t* io, size_t size, size_t per_wg, int levels) {
    hipLaunchKernelGGL(sha256_fold_multi_kernel, dim3((unsigned)(size / per_wg)), dim3(256), 0, c->stream, io, (uint32_t)size, (uint32_t)per_wg, levels);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
HashLaunchers sha256_launchers() { return {sha256_rows, sha256_fold, sha256_fold_deep<3>, sha256_fold_deep<2>, sha256_fold_small}; }

}  // namespace bx
