// circuit_common.hip — the host helpers and the two small kernels the built-in circuits share (circuit_common.hpp).
#define BX_PLAIN_MAD 1
#include "circuit_common.hpp"

namespace bx {

const char* segment_header(bx_ctx* c, const uint8_t* segment, size_t segment_len, uint32_t po2, uint64_t* seed) {
    uint32_t seg_po2 = 0;
    if (const char* e = bx_segment_decode(segment, segment_len, nullptr, &seg_po2, seed)) return set_msg(c, e);
    if (seg_po2 != po2) {
        snprintf(c->err, sizeof c->err, "prove_segment: the segment has po2 %u, this prover was created for po2 %u", seg_po2, po2);
        return c->err;
    }
    return nullptr;
}

// mixpows[i] = poly_mix^i for i < n (canonical), followed by the same table centred
__global__ void mix_table_kernel(uint32_t* __restrict__ out, Fp4 base, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fp4 r = f4_pow(base, i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        out[4 * i + k] = r.c[k];
        out[4 * (n + i) + k] = (uint32_t)fp_centre(r.c[k]);
    }
}
const char* mix_power_table(bx_ctx* c, bx_buf mixpows, const uint32_t poly_mix[4], uint32_t n) {
    BX_REQUIRE(c, mixpows.len >= 8 * (size_t)n, "circuit_mix_table: table too small");
    if (!n) return nullptr;
    hipLaunchKernelGGL(mix_table_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, (uint32_t*)mixpows.dptr,
                       Fp4{{poly_mix[0], poly_mix[1], poly_mix[2], poly_mix[3]}}, n);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}

// 1 / ((3x)^N - 1) takes four values on the domain x = w_4N^row: (3x)^N = 3^N w_4^(row mod 4)
void vanishing_inverses(uint32_t po2, uint32_t zinv[4]) {
    const uint32_t t3n = fp_pow(MONT_THREE, (uint64_t)1 << po2), w4 = fp_pow(fp_encode(137u), (uint64_t)1 << 25);  // ROU_FWD[2]
    uint32_t cur = MONT_ONE;
    for (int m = 0; m < 4; ++m) {
        zinv[m] = fp_inv(fp_sub(fp_mul(t3n, cur), MONT_ONE));
        cur = fp_mul(cur, w4);
    }
}

__global__ void ext_store_kernel(uint32_t* __restrict__ accum, const uint32_t* __restrict__ run, uint32_t po2, uint32_t n_ext, uint32_t wa,
                                 uint64_t seed) {
    const uint32_t n = 1u << po2;
    const size_t total = (size_t)n * n_ext, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t s = (uint32_t)(i >> po2), r = (uint32_t)(i & (n - 1));
        const uint4 v = *reinterpret_cast<const uint4*>(run + 4 * i);
        uint32_t* o = accum + (size_t)(4 * s) * n + r;
        o[0] = v.x; o[n] = v.y; o[2 * (size_t)n] = v.z; o[3 * (size_t)n] = v.w;
    }
    const size_t filler = (size_t)n * (wa - 4 * n_ext);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < filler; i += stride) {
        const uint32_t c = 4 * n_ext + (uint32_t)(i >> po2), r = (uint32_t)(i & (n - 1));
        accum[(size_t)c * n + r] = synth_word(seed, c, r);
    }
}
const char* store_ext_columns(bx_ctx* c, bx_buf accum, bx_buf run, uint32_t po2, uint32_t n_ext, uint32_t wa, uint64_t seed) {
    const size_t n = (size_t)1 << po2;
    hipLaunchKernelGGL(ext_store_kernel, dim3(grid_for(n * wa)), dim3(256), 0, c->stream, (uint32_t*)accum.dptr, (const uint32_t*)run.dptr, po2,
                       n_ext, wa, seed);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}

}  // namespace bx
