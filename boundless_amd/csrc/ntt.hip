// ntt.hip — batched radix-2 NTT / LDE over BabyBear for gfx950 (column-major, one polynomial per column).
//
// Entry points restate risc0_zkp::hal::Hal::{batch_interpolate_ntt, batch_evaluate_ntt,
// batch_expand_into_evaluate_ntt, batch_bit_reverse, zk_shift} (risc0-zkp 3.0.3, reference Cargo.lock:9155),
// reached from bento/crates/workflow/src/tasks/prove.rs:41-49.  The upstream CPU code is a recursive
// radix-2 DIF/DIT; the arithmetic is exact, so any factorisation of the same DFT gives identical words.
//
// MI355X design: a size-2^m transform is factored "four-step" as 2^m = 2^m_hi * 2^m_lo.
//   pass A : 2^m_lo contiguous blocks of 2^m_hi elements, transformed with perfectly coalesced loads/stores; the
//            inter-pass twist w_M^(j_lo*k2) (and the 1/M scale for the inverse) comes from a precomputed table that is
//            streamed in the same order as the data.
//   pass B : 2^m_lo-point transforms across the blocks (stride 2^m_hi), T adjacent positions per workgroup so every
//            row access is a T*4-byte contiguous segment.
// Forward (evaluate) = A then B, bit-reversed coefficients -> natural evaluations; the zero-padding "expand" is
// folded into pass A's load (out[i] = in[i >> bits]; the first `bits` stages are skipped exactly like upstream).
// Inverse (interpolate) = B then A.  Each pass moves every element through HBM once: 2 reads + 2 writes per element
// instead of m.  Sizes with m <= m_hi need pass A only.
// Two kernel families implement the passes:
//   ntt_r16.hpp  (default) register-resident radix-16 steps, LDS only for regrouping — the fast path for tiles >= 2^10;
//   this file    ntt_block_kernel / ntt_strided_kernel: one radix-2 stage per LDS round trip — the general fallback for
//                small or unaligned shapes and unusual expand_bits (tunable ntt_fast = 0 forces it; both are tested).
// Which family, compiled geometry and launch shape a pass takes is decided by ntt_plan() (ntt_plan.hpp, host-only) before the
// first launch; the host half of this file executes plans.
#include <utility>

#include "ctx.hpp"
#include "ntt_r16.hpp"

namespace bx {

// ---------------------------------------------------------------------------------------------------------
// in-LDS radix-2 stages over `rows` = 2^lr points laid out with a unit of `T` = 2^lt adjacent lanes:
// element (r, t) lives at s[r*T + t].  ltw is the stage table (ltw[half + e] = w_{2*half}^e).
// ---------------------------------------------------------------------------------------------------------
template <bool INV>
__device__ __forceinline__ void lds_stages(uint32_t* __restrict__ s, const uint32_t* __restrict__ ltw, int lr, int lt,
                                           int first_stage, int tid, int nthreads) {
    const uint32_t bfly = 1u << (lr - 1 + lt);
    const uint32_t tmask = (1u << lt) - 1u;
    if (!INV) {
        for (int stage = first_stage; stage <= lr; ++stage) {
            const uint32_t half = 1u << (stage - 1);
            for (uint32_t x = tid; x < bfly; x += nthreads) {
                uint32_t t = x & tmask, q = x >> lt;
                uint32_t lo = q & (half - 1u);
                uint32_t i = (((q - lo) << 1) | lo);
                uint32_t ia = (i << lt) | t, ib = ((i + half) << lt) | t;
                uint32_t a = s[ia];
                uint32_t b = fp_mul(s[ib], ltw[half + lo]);
                s[ia] = fp_add(a, b);
                s[ib] = fp_sub(a, b);
            }
            __syncthreads();
        }
    } else {
        for (int stage = lr; stage >= 1; --stage) {
            const uint32_t half = 1u << (stage - 1);
            for (uint32_t x = tid; x < bfly; x += nthreads) {
                uint32_t t = x & tmask, q = x >> lt;
                uint32_t lo = q & (half - 1u);
                uint32_t i = (((q - lo) << 1) | lo);
                uint32_t ia = (i << lt) | t, ib = ((i + half) << lt) | t;
                uint32_t a = s[ia], b = s[ib];
                s[ia] = fp_add(a, b);
                s[ib] = fp_mul(fp_sub(a, b), ltw[half + lo]);
            }
            __syncthreads();
        }
    }
}

// pass A: one workgroup per (block, column).  LDS = data[R] + stage table[R].
template <bool INV>
__global__ void ntt_block_kernel(uint32_t* out, const uint32_t* in,  // may alias (in-place): no __restrict__
                                 const uint32_t* __restrict__ tw, const uint32_t* __restrict__ twist, uint32_t scale,
                                 int lr, int expand_bits, int first_stage, size_t in_col_stride, size_t out_col_stride) {
    extern __shared__ uint32_t lds[];
    const uint32_t R = 1u << lr;
    uint32_t* s = lds;
    uint32_t* ltw = lds + R;
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t block = blockIdx.x, col = blockIdx.y;
    const uint32_t* src = in + col * in_col_stride + ((block << lr) >> expand_bits);
    uint32_t* dst = out + col * out_col_stride + (block << lr);
    const uint32_t* twb = twist ? twist + (block << lr) : nullptr;

    for (uint32_t i = tid; i < R; i += nt) ltw[i] = tw[i];
    if (!INV) {
        for (uint32_t i = tid; i < R; i += nt) s[i] = src[i >> expand_bits];
        __syncthreads();
        lds_stages<false>(s, ltw, lr, 0, first_stage, tid, nt);
        if (twb) {
            for (uint32_t i = tid; i < R; i += nt) dst[i] = fp_mul(s[i], twb[i]);
        } else {
            for (uint32_t i = tid; i < R; i += nt) dst[i] = s[i];
        }
    } else {
        if (twb) {
            for (uint32_t i = tid; i < R; i += nt) s[i] = fp_mul(src[i], twb[i]);
        } else {
            for (uint32_t i = tid; i < R; i += nt) s[i] = fp_mul(src[i], scale);
        }
        __syncthreads();
        lds_stages<true>(s, ltw, lr, 0, 1, tid, nt);
        for (uint32_t i = tid; i < R; i += nt) dst[i] = s[i];
    }
}

// pass B: one workgroup per (tile of T adjacent positions, column); rows are 2^m_hi apart.  In place.
// `tile_swz`: blockIdx.x -> tile remap so that tiles sharing a 128-byte line run on the same XCD (block b is
// observed on XCD b % 8; a performance hint only).
template <bool INV>
__global__ void ntt_strided_kernel(uint32_t* __restrict__ io, const uint32_t* __restrict__ tw, int lr, int lt, int m_hi,
                                   size_t col_stride, uint32_t tiles) {
    extern __shared__ uint32_t lds[];
    const uint32_t rows = 1u << lr, T = 1u << lt;
    uint32_t* s = lds;
    uint32_t* ltw = lds + (rows << lt);
    const int tid = threadIdx.x, nt = blockDim.x;
    uint32_t b = blockIdx.x;
    uint32_t tile = (tiles % 8u == 0u) ? (b % 8u) * (tiles / 8u) + b / 8u : b;
    uint32_t* base = io + (size_t)blockIdx.y * col_stride + ((size_t)tile << lt);
    const uint32_t total = rows << lt, tmask = T - 1u;

    for (uint32_t i = tid; i < rows; i += nt) ltw[i] = tw[i];
    for (uint32_t e = tid; e < total; e += nt) s[e] = base[((size_t)(e >> lt) << m_hi) + (e & tmask)];
    __syncthreads();
    lds_stages<INV>(s, ltw, lr, lt, 1, tid, nt);
    for (uint32_t e = tid; e < total; e += nt) base[((size_t)(e >> lt) << m_hi) + (e & tmask)] = s[e];
}

// twist[b*2^m_hi + i] = w_M^(+-rev_{m_lo}(b) * i) (* 1/M for the inverse)
__global__ void twist_build_kernel(uint32_t* __restrict__ out, uint32_t root, uint32_t scale, int m, int m_hi) {
    size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= ((size_t)1 << m)) return;
    uint32_t b = (uint32_t)(p >> m_hi), i = (uint32_t)(p & (((size_t)1 << m_hi) - 1));
    uint64_t e = ((uint64_t)bit_reverse(b, m - m_hi) * i) & (((uint64_t)1 << m) - 1);
    out[p] = fp_mul(fp_pow(root, e), scale);
}

__global__ void zk_tab_kernel(uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, int n, int lo_bits) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (1u << lo_bits)) lo[i] = fp_pow(MONT_THREE, (uint64_t)bit_reverse(i, lo_bits) << (n - lo_bits));
    if (i < (1u << (n - lo_bits))) hi[i] = fp_pow(MONT_THREE, bit_reverse(i, n - lo_bits));
}
__global__ void zk_shift_kernel(uint32_t* __restrict__ io, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                int n, int lo_bits, size_t total) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        uint32_t pos = (uint32_t)(i & (((size_t)1 << n) - 1));
        uint32_t f = fp_mul(lo[pos & ((1u << lo_bits) - 1u)], hi[pos >> lo_bits]);
        io[i] = fp_mul(io[i], f);
    }
}
__global__ void bit_reverse_kernel(uint32_t* __restrict__ io, int n, size_t total) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        uint32_t i = (uint32_t)(g & (((size_t)1 << n) - 1));
        uint32_t r = bit_reverse(i, n);
        if (i < r) {
            size_t base = g - i;
            uint32_t a = io[base + i], b = io[base + r];
            io[base + i] = b;
            io[base + r] = a;
        }
    }
}

// Tiled bit reversal for n >= 12: index i = (a:6 | b:n-12 | c:6) maps to (rev c | rev b | rev a), so the 64x64 tile
// {all a, all c} with middle bits b lands, transposed, on the tile with middle bits rev(b).  A workgroup loads the pair
// (b, rev b), swaps the two tiles through LDS and stores them: each word moves HBM->HBM once.  Every lane moves 16 bytes per
// access (a wave instruction covers four 256-byte rows) and all eight loads of a thread are issued before the first LDS write:
// with one word per lane the launch had too few bytes in flight to cover the HBM latency (28 % of the roofline).
__global__ __launch_bounds__(256) void bit_reverse_tiled_kernel(uint32_t* __restrict__ io, int n) {
    __shared__ uint32_t A[64][65], B[64][65];
    const int nb = n - 12;
    const uint32_t b = blockIdx.x, rb = bit_reverse(b, nb);
    if (rb < b) return;
    uint32_t* col = io + ((size_t)blockIdx.y << n);
    const uint32_t l16 = threadIdx.x & 15u, r = threadIdx.x >> 4;  // lane: words 4 l16 .. 4 l16 + 3 of row r + 16 p
    const int hs = n - 6;
    const bool two = rb != b;
    uint4 va[4], vb[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const size_t row = (size_t)(r + 16u * p) << hs;
        va[p] = *reinterpret_cast<const uint4*>(col + row + (b << 6) + 4u * l16);
        if (two) vb[p] = *reinterpret_cast<const uint4*>(col + row + (rb << 6) + 4u * l16);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        uint32_t* ar = &A[r + 16u * p][4u * l16];
        ar[0] = va[p].x, ar[1] = va[p].y, ar[2] = va[p].z, ar[3] = va[p].w;
        if (two) {
            uint32_t* br = &B[r + 16u * p][4u * l16];
            br[0] = vb[p].x, br[1] = vb[p].y, br[2] = vb[p].z, br[3] = vb[p].w;
        }
    }
    __syncthreads();
    // output word c = 4 l16 + i of row a comes from A[rev6(c)][rev6(a)], and rev6(4 l16 + i) = 16 rev2(i) + rev4(l16)
    const uint32_t s0 = bit_reverse(l16, 4);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t a = r + 16u * p, ra = bit_reverse(a, 6);
        const size_t row = (size_t)a << hs;
        *reinterpret_cast<uint4*>(col + row + (rb << 6) + 4u * l16) = make_uint4(A[s0][ra], A[32u + s0][ra], A[16u + s0][ra], A[48u + s0][ra]);
        if (two) *reinterpret_cast<uint4*>(col + row + (b << 6) + 4u * l16) = make_uint4(B[s0][ra], B[32u + s0][ra], B[16u + s0][ra], B[48u + s0][ra]);
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
const char* ntt_init_tables(bx_ctx* c) {
    const size_t n = (size_t)1 << TW_LOG;
    std::vector<uint32_t> f(n, 0), r(n, 0);
    uint32_t rou[28], rev[28];
    rou[27] = fp_encode(137u);
    for (int k = 26; k >= 0; --k) rou[k] = fp_mul(rou[k + 1], rou[k + 1]);
    for (int k = 0; k < 28; ++k) rev[k] = fp_inv(rou[k]);
    for (int s = 1; s <= TW_LOG; ++s) {
        size_t half = (size_t)1 << (s - 1);
        uint32_t cf = MONT_ONE, cr = MONT_ONE;
        for (size_t e = 0; e < half; ++e) {
            f[half + e] = cf;
            r[half + e] = cr;
            cf = fp_mul(cf, rou[s]);
            cr = fp_mul(cr, rev[s]);
        }
    }
    BX_HIP(c, hipMalloc(&c->d_tw_fwd, n * 4));
    BX_HIP(c, hipMalloc(&c->d_tw_inv, n * 4));
    BX_HIP(c, hipMemcpy(c->d_tw_fwd, f.data(), n * 4, hipMemcpyHostToDevice));
    BX_HIP(c, hipMemcpy(c->d_tw_inv, r.data(), n * 4, hipMemcpyHostToDevice));
    return nullptr;
}
void ntt_free_tables(bx_ctx* c) {
    if (c->d_tw_fwd) (void)hipFree(c->d_tw_fwd);
    if (c->d_tw_inv) (void)hipFree(c->d_tw_inv);
    for (auto& kv : c->twist) (void)hipFree(kv.second);
    for (auto& kv : c->zk) {
        (void)hipFree(kv.second.lo);
        (void)hipFree(kv.second.hi);
    }
    for (auto& kv : c->zk_full) (void)hipFree(kv.second);
    c->twist.clear();
    c->zk.clear();
    c->zk_full.clear();
}

static const char* get_twist(bx_ctx* c, int m, int m_hi, bool inverse, uint32_t** out) {
    TwistKey key{m, m_hi, inverse ? 1 : 0};
    auto it = c->twist.find(key);
    if (it != c->twist.end()) {
        *out = it->second;
        return nullptr;
    }
    uint32_t* d = nullptr;
    size_t M = (size_t)1 << m;
    BX_HIP(c, hipMalloc(&d, M * 4));
    uint32_t root = fp_pow(fp_encode(137u), (uint64_t)1 << (27 - m));  // w_M
    uint32_t scale = MONT_ONE;
    if (inverse) {
        root = fp_inv(root);
        scale = fp_inv(fp_encode((uint32_t)M));
    }
    hipLaunchKernelGGL(twist_build_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, d, root, scale, m,
                       m_hi);
    BX_LAUNCH_CHECK(c);
    c->twist[key] = d;
    *out = d;
    return nullptr;
}

template <typename K>
static const char* allow_lds(bx_ctx* c, K kernel, size_t bytes) {
    if (bytes > 64 * 1024) BX_HIP(c, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return nullptr;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ---- executing a plan (ntt_plan.hpp): which kernel runs, and in what shape, was decided before the first launch ----------
using R16Kernel = void (*)(R16Args);

// ntt_r16_kernel<INV, PASS_A, SKIP, ..> of every row of NTT_GEOMS: the one place a row index becomes an instantiation
template <bool INV, bool PASS_A, int SKIP, size_t... I>
static R16Kernel r16_row(int geom, std::index_sequence<I...>) {
    static const R16Kernel rows[] = {ntt_r16_kernel<INV, PASS_A, SKIP, NTT_GEOMS[I].lr, NTT_GEOMS[I].lt, NTT_GEOMS[I].maxt>...};
    return rows[geom];
}
static R16Kernel r16_geom_kernel(bool inv, bool pass_a, int skip, int geom) {
    constexpr auto rows = std::make_index_sequence<NTT_GEOM_COUNT>();
    if (!pass_a) return inv ? r16_row<true, false, 0>(geom, rows) : r16_row<false, false, 0>(geom, rows);
    if (inv) return r16_row<true, true, 0>(geom, rows);
    return skip == 2 ? r16_row<false, true, 2>(geom, rows) : r16_row<false, true, 0>(geom, rows);
}

// a planned radix-16 pass: `a` holds the buffers, strides and factors, the plan everything else
static const char* launch_r16_pass(bx_ctx* c, const NttPass& p, bool inv, bool pass_a, int skip, size_t count, R16Args a) {
    a.tw = inv ? c->d_tw_inv : c->d_tw_fwd;
    a.lr = p.lr; a.lrows = p.lrows; a.lt = p.lt; a.row_shift = p.row_shift;
    a.tiles = p.tiles; a.cols = (uint32_t)count; a.cpw = p.cpw;
    if (p.family == NTT_MULTI_A) {
        const R16Kernel multi_kernel = skip == 2 ? ntt_passA_fwd12_multi_kernel<2> : ntt_passA_fwd12_multi_kernel<0>;
        hipLaunchKernelGGL(multi_kernel, dim3(p.grid_x), dim3(p.threads), p.lds, c->stream, a);
    } else {
        const R16Kernel r16_kernel = r16_geom_kernel(inv, pass_a, skip, p.geom);
        BX_TRY(allow_lds(c, r16_kernel, p.lds));
        hipLaunchKernelGGL(r16_kernel, dim3(p.grid_x), dim3(p.threads), p.lds, c->stream, a);
    }
    BX_LAUNCH_CHECK(c);
    return nullptr;
}

// Pass A of plan `p` over its columns.  Forward: in (2^m >> expand words per column) -> out, `skip` leading stages skipped, times the
// twist.  Inverse: in place, times the twist (or `scale` = 1/M where there is no pass B), and times `post` on the final store where
// the plan says so.
static const char* launch_pass_a(bx_ctx* c, const NttPlan& p, bool inv, uint32_t* out, const uint32_t* in, const uint32_t* twist,
                                 uint32_t scale, const uint32_t* post, int m, int expand, int skip) {
    const size_t M = (size_t)1 << m;
    if (p.a.family == NTT_V1) {
        const auto block_kernel = inv ? ntt_block_kernel<true> : ntt_block_kernel<false>;
        BX_TRY(allow_lds(c, block_kernel, p.a.lds));
        hipLaunchKernelGGL(block_kernel, dim3(p.a.grid_x, p.a.grid_y), dim3(p.a.threads), p.a.lds, c->stream, out, in,
                           inv ? c->d_tw_inv : c->d_tw_fwd, twist, scale, p.a.lr, expand, skip + 1, M >> expand, M);
        BX_LAUNCH_CHECK(c);
        return nullptr;
    }
    R16Args a;
    a.out = out; a.in = in; a.twist = twist; a.scale = scale;
    a.post = p.post_on_a ? post : nullptr;
    a.expand = expand;
    a.tile_stride = 1u << p.a.lrows;
    a.in_col_stride = M >> expand; a.out_col_stride = M;
    return launch_r16_pass(c, p.a, inv, true, skip, p.count, a);
}

// Pass B of plan `p` over its columns, in place.
static const char* launch_pass_b(bx_ctx* c, const NttPlan& p, bool inv, uint32_t* io, int m) {
    const size_t M = (size_t)1 << m;
    if (p.b.family == NTT_V1) {
        const auto strided_kernel = inv ? ntt_strided_kernel<true> : ntt_strided_kernel<false>;
        BX_TRY(allow_lds(c, strided_kernel, p.b.lds));
        hipLaunchKernelGGL(strided_kernel, dim3(p.b.grid_x, p.b.grid_y), dim3(p.b.threads), p.b.lds, c->stream, io,
                           inv ? c->d_tw_inv : c->d_tw_fwd, p.b.lr, p.b.lt, p.m_hi, M, p.b.tiles);
        BX_LAUNCH_CHECK(c);
        return nullptr;
    }
    R16Args a;
    a.out = io; a.in = io; a.twist = nullptr; a.scale = MONT_ONE;
    a.expand = 0;
    a.tile_stride = 1u << p.b.lt;
    a.in_col_stride = a.out_col_stride = M;
    return launch_r16_pass(c, p.b, inv, false, 0, p.count, a);
}

// forward transform of `count` columns: in (size M >> expand_bits per column) -> out (size M per column), A then B.
// `expand_bits` = load shift (out[i] = in[i >> bits]); `skip_bits` = leading stages skipped (== expand_bits for the
// expanding form, and for the in-place Hal::batch_evaluate_ntt(io, count, expand_bits) with no load shift).
// With ntt_group_cols the two passes run on a group of columns at a time (ntt_forward_group); the plan of a full group and the plan
// of the ragged last one are both made before the first launch.
static const char* forward(bx_ctx* c, uint32_t* out, const uint32_t* in, size_t count, int m, int expand_bits,
                           int skip_bits) {
    if (m == 0 || count == 0) {
        if (out != in) BX_HIP(c, hipMemcpyAsync(out, in, count * 4, hipMemcpyDeviceToDevice, c->stream));
        return nullptr;
    }
    const bool al = aligned16(out) && aligned16(in);
    const size_t g = ntt_forward_group(c->ntt, m, expand_bits, skip_bits, count, al);
    const NttPlan full = ntt_plan(c->ntt, false, m, expand_bits, skip_bits, g, al, false);
    const NttPlan last = count % g ? ntt_plan(c->ntt, false, m, expand_bits, skip_bits, count % g, al, false) : full;
    BX_REQUIRE(c, !full.error, full.error);
    BX_REQUIRE(c, !last.error, last.error);
    const size_t M = (size_t)1 << m;
    uint32_t* twist = nullptr;
    if (full.twist) BX_TRY(get_twist(c, m, full.m_hi, false, &twist));
    for (size_t c0 = 0; c0 < count; c0 += g) {
        const NttPlan& p = count - c0 < g ? last : full;
        BX_TRY(launch_pass_a(c, p, false, out + c0 * M, in + c0 * (M >> expand_bits), twist, MONT_ONE, nullptr, m, expand_bits, skip_bits));
        if (p.m_lo) BX_TRY(launch_pass_b(c, p, false, out + c0 * M, m));
    }
    return nullptr;
}

// inverse transform in place by plan `p` (m >= 1): B then A.  `post`: the factor table of a plan with post_on_a.
static const char* inverse(bx_ctx* c, const NttPlan& p, uint32_t* io, int m, const uint32_t* post) {
    uint32_t* twist = nullptr;
    if (p.twist) BX_TRY(get_twist(c, m, p.m_hi, true, &twist));
    if (p.m_lo) BX_TRY(launch_pass_b(c, p, true, io, m));
    const uint32_t scale = fp_inv(fp_encode((uint32_t)((size_t)1 << m)));
    return launch_pass_a(c, p, true, io, io, twist, scale, post, m, 0, 0);
}

static const char* get_zk(bx_ctx* c, int n, ZkTab* out) {
    auto it = c->zk.find(n);
    if (it != c->zk.end()) {
        *out = it->second;
        return nullptr;
    }
    ZkTab t;
    t.lo_bits = (n + 1) / 2;
    size_t nlo = (size_t)1 << t.lo_bits, nhi = (size_t)1 << (n - t.lo_bits);
    BX_HIP(c, hipMalloc(&t.lo, nlo * 4));
    BX_HIP(c, hipMalloc(&t.hi, nhi * 4));
    hipLaunchKernelGGL(zk_tab_kernel, dim3((unsigned)((nlo + 255) / 256)), dim3(256), 0, c->stream, t.lo, t.hi, n, t.lo_bits);
    BX_LAUNCH_CHECK(c);
    c->zk[n] = t;
    *out = t;
    return nullptr;
}

__global__ void zk_full_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, int n,
                               int lo_bits) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ((size_t)1 << n)) out[i] = fp_mul(lo[i & ((1u << lo_bits) - 1u)], hi[i >> lo_bits]);
}
// 3^bitrev_n(i) for every position of a size-2^n column (4 MB at n = 20, read through L2 by the fused inverse pass)
static const char* get_zk_full(bx_ctx* c, int n, const uint32_t** out) {
    auto it = c->zk_full.find(n);
    if (it != c->zk_full.end()) {
        *out = it->second;
        return nullptr;
    }
    ZkTab t;
    BX_TRY(get_zk(c, n, &t));
    uint32_t* full = nullptr;
    BX_HIP(c, hipMalloc(&full, ((size_t)1 << n) * 4));
    hipLaunchKernelGGL(zk_full_kernel, dim3((unsigned)((((size_t)1 << n) + 255) / 256)), dim3(256), 0, c->stream, full, t.lo, t.hi, n,
                       t.lo_bits);
    BX_LAUNCH_CHECK(c);
    c->zk_full[n] = full;
    *out = full;
    return nullptr;
}

}  // namespace bx

using namespace bx;

static const char* zk_shift_impl(bx_ctx* c, bx_buf io, size_t count);

// Extension: batch_interpolate_ntt followed by zk_shift in one call.  When the register-radix path covers the shape the
// shift rides on the final store of the inverse transform (one extra product per element instead of a read-modify-write
// pass over the coefficients); otherwise it is the two calls.
extern "C" const char* bx_batch_interpolate_zk(bx_ctx* c, bx_buf io, size_t count) try {
    if (!c) return "bx_batch_interpolate_zk: null ctx";
    BX_REQUIRE(c, count > 0 && io.len % count == 0 && is_pow2(io.len / count), "batch_interpolate_zk: io.len/count must be a power of two");
    BX_ENTER(c);
    const int m = ilog2(io.len / count);
    NttPlan p;
    {
        OpScope op(c, "batch_interpolate_ntt", 8.0 * (double)io.len);
        if (m > 0) {
            // the 2^m-word table of factors is worth building from 2^12 on, and is built only where the plan uses it
            p = ntt_plan(c->ntt, true, m, 0, 0, count, aligned16(io.dptr), m >= 12);
            BX_REQUIRE(c, !p.error, p.error);
            const uint32_t* post = nullptr;
            if (p.post_on_a) BX_TRY(get_zk_full(c, m, &post));
            BX_TRY(inverse(c, p, (uint32_t*)io.dptr, m, post));
        }
    }
    if (p.post_on_a) return nullptr;
    return zk_shift_impl(c, io, count);
} BX_ABI_CATCH(c, "bx_batch_interpolate_zk")

extern "C" const char* bx_batch_interpolate_ntt(bx_ctx* c, bx_buf io, size_t count) try {
    if (!c) return "bx_batch_interpolate_ntt: null ctx";
    BX_REQUIRE(c, count > 0 && io.len % count == 0 && is_pow2(io.len / count), "batch_interpolate_ntt: io.len/count must be a power of two");
    BX_ENTER(c);
    OpScope op(c, "batch_interpolate_ntt", 8.0 * (double)io.len);
    const int m = ilog2(io.len / count);
    if (m == 0) return nullptr;
    const NttPlan p = ntt_plan(c->ntt, true, m, 0, 0, count, aligned16(io.dptr), false);
    BX_REQUIRE(c, !p.error, p.error);
    return inverse(c, p, (uint32_t*)io.dptr, m, nullptr);
} BX_ABI_CATCH(c, "bx_batch_interpolate_ntt")

extern "C" const char* bx_batch_evaluate_ntt(bx_ctx* c, bx_buf io, size_t count, size_t expand_bits) try {
    if (!c) return "bx_batch_evaluate_ntt: null ctx";
    BX_REQUIRE(c, count > 0 && io.len % count == 0 && is_pow2(io.len / count), "batch_evaluate_ntt: io.len/count must be a power of two");
    int m = ilog2(io.len / count);
    BX_REQUIRE(c, expand_bits <= (size_t)m, "batch_evaluate_ntt: expand_bits > log2(size)");
    BX_ENTER(c);
    OpScope op(c, "batch_evaluate_ntt", 8.0 * (double)io.len);
    return forward(c, (uint32_t*)io.dptr, (const uint32_t*)io.dptr, count, m, 0, (int)expand_bits);
} BX_ABI_CATCH(c, "bx_batch_evaluate_ntt")

extern "C" const char* bx_batch_expand_into_evaluate_ntt(bx_ctx* c, bx_buf out, bx_buf in, size_t count, size_t expand_bits) try {
    if (!c) return "bx_batch_expand_into_evaluate_ntt: null ctx";
    BX_REQUIRE(c, count > 0 && in.len % count == 0 && is_pow2(in.len / count), "batch_expand_into_evaluate_ntt: in.len/count must be a power of two");
    BX_REQUIRE(c, expand_bits < 32 && out.len >> expand_bits == in.len && out.len == (in.len << expand_bits), "batch_expand_into_evaluate_ntt: out.len != in.len << expand_bits");
    // the expansion reads in[i >> bits] while other lanes write out: only the transform in place (no expansion) may share memory
    BX_REQUIRE(c, (expand_bits == 0 && bufs_same(out, in)) || !bufs_overlap(out, in), "batch_expand_into_evaluate_ntt: out and in overlap");
    BX_ENTER(c);
    OpScope op(c, "batch_expand_into_evaluate_ntt", 4.0 * (double)in.len + 4.0 * (double)out.len);
    int m = ilog2(out.len / count);
    return forward(c, (uint32_t*)out.dptr, (const uint32_t*)in.dptr, count, m, (int)expand_bits, (int)expand_bits);
} BX_ABI_CATCH(c, "bx_batch_expand_into_evaluate_ntt")

extern "C" const char* bx_batch_bit_reverse(bx_ctx* c, bx_buf io, size_t count) try {
    if (!c) return "bx_batch_bit_reverse: null ctx";
    BX_REQUIRE(c, count > 0 && io.len % count == 0 && is_pow2(io.len / count), "batch_bit_reverse: io.len/count must be a power of two");
    BX_ENTER(c);
    OpScope op(c, "batch_bit_reverse", 8.0 * (double)io.len);
    int n = ilog2(io.len / count);
    if (n == 0) return nullptr;
    if (n >= 12 && n <= 30 && ((uintptr_t)io.dptr & 15u) == 0) {  // the tiled kernel moves 16 bytes per lane
        hipLaunchKernelGGL(bit_reverse_tiled_kernel, dim3(1u << (n - 12), (unsigned)count), dim3(256), 0, c->stream,
                           (uint32_t*)io.dptr, n);
        BX_LAUNCH_CHECK(c);
        return nullptr;
    }
    size_t blocks = (io.len + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(bit_reverse_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, (uint32_t*)io.dptr, n, io.len);
    BX_LAUNCH_CHECK(c);
    return nullptr;
} BX_ABI_CATCH(c, "bx_batch_bit_reverse")

// Bit reversal of AoS extension-field arrays (16-byte elements): one thread swaps element i with element rev(i), i < rev(i).
__global__ void bit_reverse_ext_kernel(uint4* __restrict__ io, int n, size_t total) {
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)(g & (((size_t)1 << n) - 1));
        const uint32_t r = bit_reverse(i, n);
        if (i < r) {
            uint4* base = io + (g - i);
            const uint4 a = base[i], b = base[r];
            base[i] = b;
            base[r] = a;
        }
    }
}
extern "C" const char* bx_batch_bit_reverse_ext(bx_ctx* c, bx_buf io_ext, size_t count) try {
    if (!c) return "bx_batch_bit_reverse_ext: null ctx";
    BX_REQUIRE(c, count > 0 && count <= io_ext.len / 4 && io_ext.len % (4 * count) == 0 && is_pow2(io_ext.len / (4 * count)),
               "batch_bit_reverse_ext: io.len/(4*count) must be a power of two");
    BX_REQUIRE(c, ((uintptr_t)io_ext.dptr & 15) == 0, "batch_bit_reverse_ext: buffer must be 16-byte aligned");
    BX_ENTER(c);
    OpScope op(c, "batch_bit_reverse", 8.0 * (double)io_ext.len);
    const size_t elems = io_ext.len / 4;
    const int n = ilog2(elems / count);
    if (n == 0) return nullptr;
    size_t blocks = (elems + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(bit_reverse_ext_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, (uint4*)io_ext.dptr, n, elems);
    BX_LAUNCH_CHECK(c);
    return nullptr;
} BX_ABI_CATCH(c, "bx_batch_bit_reverse_ext")

extern "C" const char* bx_zk_shift(bx_ctx* c, bx_buf io, size_t count) try {
    if (!c) return "bx_zk_shift: null ctx";
    return zk_shift_impl(c, io, count);
} BX_ABI_CATCH(c, "bx_zk_shift")
static const char* zk_shift_impl(bx_ctx* c, bx_buf io, size_t count) {
    BX_REQUIRE(c, count > 0 && io.len % count == 0 && is_pow2(io.len / count), "zk_shift: io.len/count must be a power of two");
    BX_ENTER(c);
    OpScope op(c, "zk_shift", 8.0 * (double)io.len);
    int n = ilog2(io.len / count);
    ZkTab t;
    BX_TRY(get_zk(c, n, &t));
    size_t blocks = (io.len + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(zk_shift_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, (uint32_t*)io.dptr, t.lo, t.hi, n,
                       t.lo_bits, io.len);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
