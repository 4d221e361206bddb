// bn254.hip — the BN254 Groth16 prover on gfx950: Pippenger MSM over G1 / G2, the Fr NTT on the odd coset, the coefficient
// evaluation kernels, key upload and the per-proof orchestration (include/bx_groth16.h; conventions in groth16.hpp and
// bn254_arith.hpp).
//
// MSM (msm_run): window width c by n; W = ceil(256 / c) windows, buckets (w, d) with d in [1, 2^c).
//   1. msm_count: one lane per point, one atomic per non-zero digit into the bucket histogram (zero scalars and points at infinity
//      add nothing);  2. scan (three-phase, u32) -> bucket offsets;  3. msm_scatter: point indices sorted by bucket (counting sort);
//   4. bucket sums by levels: each bucket's list is cut into chunks of CHUNK entries, one lane per chunk (level 0: mixed affine
//      additions; later levels: XYZZ additions of the previous level's partial sums), until every bucket has one partial — a
//      skewed bucket (circom witnesses are mostly 0 and 1) is summed by many lanes, not one;
//   5. msm_window_reduce: G = 2^c / 2048 workgroups per window (at least 1), 256 lanes each owning a segment of buckets: sum k * B_k
//      by running sums within the segment plus (lo - 1) * (segment sum), a tree over the lanes in LDS, then msm_window_sum: a tree
//      over the G partials of each window;  6. on the host (msm_entry): Horner over the W window sums, affine.
//   The histogram and the scatter aggregate the lanes of a wave that hit the same bucket as the wave's first non-zero digit into one
//   atomic, so the one bucket that a circom witness's many 1s fall into is not a chain of single atomics.
// NTT: radix-2; stages whose butterflies span more than 1024 elements run one launch each on global memory, the others in one LDS
//   kernel.  Inverse = decimation in frequency (natural in, bit-reversed out) with omega^-1; the odd-coset shift and 1/N are applied
//   in bit-reversed order; forward = decimation in time (bit-reversed in, natural out).  No permutation pass.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <sys/random.h>

#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "bn254_arith.hpp"
#include "ctx.hpp"
#include "groth16.hpp"

using namespace bn;

namespace {

constexpr uint32_t CHUNK = 16;  // bucket-list entries per lane and level
constexpr int SCAN_TILE = 1024;

// ---------------- scan (exclusive, u32; out has n + 1 entries, out[n] = total) ----------------
__global__ __launch_bounds__(256) void scan_tile_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ bsum,
                                                        uint32_t n) {
    __shared__ uint32_t s[256];
    const uint32_t t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + 4 * t;
    uint32_t v[4], tot = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = base + k < n ? in[base + k] : 0u;
        tot += v[k];
    }
    s[t] = tot;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        uint32_t x = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    uint32_t run = s[t] - tot;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
    if (t == 255) bsum[blockIdx.x] = s[255];
}

__global__ __launch_bounds__(256) void scan_bsum_kernel(uint32_t* __restrict__ bsum, uint32_t nblk, uint32_t* __restrict__ total) {
    __shared__ uint32_t s[256];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblk; base += 256) {
        uint32_t v = base + t < nblk ? bsum[base + t] : 0u;
        s[t] = v;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {
            uint32_t x = t >= off ? s[t - off] : 0u;
            __syncthreads();
            s[t] += x;
            __syncthreads();
        }
        if (base + t < nblk) bsum[base + t] = carry + s[t] - v;
        carry += s[255];
        __syncthreads();
    }
    if (t == 0) *total = carry;
}

__global__ void scan_add_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ bsum, uint32_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += bsum[i / SCAN_TILE];
}

// ---------------- MSM ----------------
__device__ __forceinline__ uint32_t digit(const uint32_t* s, uint32_t w, uint32_t c) {
    uint32_t bit = w * c, word = bit >> 5, sh = bit & 31;
    uint32_t v = s[word] >> sh;
    if (sh + c > 32 && word + 1 < 8) v |= s[word + 1] << (32 - sh);
    return v & ((1u << c) - 1u);
}

template <class F>
__device__ __forceinline__ Aff<F> load_aff(const uint32_t* pts, size_t i) {
    Aff<F> a;
    memcpy(&a, pts + i * (sizeof(Aff<F>) / 4), sizeof(Aff<F>));
    return a;
}

// One lane per point, one pass per window.  The lanes of a wave that share the bucket of the wave's first non-zero digit are
// served by ONE atomic (a circom witness puts ~45 % of its scalars, all digit 1 of window 0, into one bucket: unaggregated those
// atomics serialise); every other lane adds its own.  scatter = false: histogram into cnt; true: positions from cnt (the cursors).
template <class F, bool SCATTER>
__global__ __launch_bounds__(256) void msm_bucket_kernel(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ sc, uint32_t n, uint32_t c,
                                                         uint32_t W, uint32_t* __restrict__ cnt, uint32_t* __restrict__ sorted) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;  // whole lanes only leave here; every remaining lane takes part in the ballots below
    const bool live = !aff_is_inf(load_aff<F>(pts, i));
    uint32_t s[8];
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = live ? sc[(size_t)i * 8 + k] : 0u;
    const uint32_t lane = __lane_id();
    const uint64_t below = (lane ? ~0ull >> (64 - lane) : 0ull);
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t d = digit(s, w, c), b = (w << c) | d;
        const uint64_t any = __ballot(d != 0);
        if (!any) continue;
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)any) - 1;
        const uint32_t lb = __shfl(b, (int)leader);
        const bool peer = d != 0 && b == lb;
        const uint64_t peers = __ballot(peer);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&cnt[lb], (uint32_t)__popcll(peers));
        if (SCATTER) {
            base = __shfl(base, (int)leader);
            if (peer) sorted[base + (uint32_t)__popcll(peers & below)] = i;
            else if (d) sorted[atomicAdd(&cnt[b], 1u)] = i;
        } else if (d && !peer) {
            atomicAdd(&cnt[b], 1u);
        }
    }
}

// chunks per bucket of a level whose lists are given by the exclusive offsets `off` (nb + 1 entries)
__global__ void msm_chunk_count_kernel(const uint32_t* __restrict__ off, uint32_t nb, uint32_t* __restrict__ nch) {
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nb) nch[b] = (off[b + 1] - off[b] + CHUNK - 1) / CHUNK;
}

// the bucket of chunk t: the largest b with choff[b] <= t (choff[nb] > t)
__device__ __forceinline__ uint32_t chunk_bucket(const uint32_t* choff, uint32_t nb, uint32_t t) {
    uint32_t lo = 0, hi = nb;  // choff[lo] <= t < choff[hi]
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (choff[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <class F>
__global__ __launch_bounds__(256) void msm_level0_kernel(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ sorted,
                                                         const uint32_t* __restrict__ off, const uint32_t* __restrict__ choff, uint32_t nb,
                                                         Xyzz<F>* __restrict__ out) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= choff[nb]) return;
    uint32_t b = chunk_bucket(choff, nb, t);
    uint32_t beg = off[b] + (t - choff[b]) * CHUNK, end = min(off[b + 1], beg + CHUNK);
    Xyzz<F> acc = xyzz_inf<F>();
    for (uint32_t e = beg; e < end; e++) acc = xyzz_add_aff(acc, load_aff<F>(pts, sorted[e]));
    out[t] = acc;
}

template <class F>
__global__ __launch_bounds__(256) void msm_level_kernel(const Xyzz<F>* __restrict__ in, const uint32_t* __restrict__ off,
                                                        const uint32_t* __restrict__ choff, uint32_t nb, Xyzz<F>* __restrict__ out) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= choff[nb]) return;
    uint32_t b = chunk_bucket(choff, nb, t);
    uint32_t beg = off[b] + (t - choff[b]) * CHUNK, end = min(off[b + 1], beg + CHUNK);
    Xyzz<F> acc = in[beg];
    for (uint32_t e = beg + 1; e < end; e++) acc = xyzz_add(acc, in[e]);
    out[t] = acc;
}

// Sum_d d * B_d of window w = blockIdx.x, split over gridDim.y workgroups of 256 lanes: lane t of workgroup g owns the buckets
// [lo, hi) of segment g * 256 + t and computes sum (d - lo + 1) B_d by running sums, plus (lo - 1) * (its sum of B_d); the lanes of a
// workgroup are then added by a tree in LDS.  Bucket (w, d) holds at most one partial: part[off[b]] when off[b + 1] > off[b].
template <class F>
__global__ __launch_bounds__(256) void msm_window_reduce_kernel(const Xyzz<F>* __restrict__ part, const uint32_t* __restrict__ off, uint32_t c,
                                                                Xyzz<F>* __restrict__ wpart) {
    __shared__ Xyzz<F> sh[256];
    const uint32_t w = blockIdx.x, t = threadIdx.x, nbw = 1u << c, lanes = 256u * gridDim.y;
    const uint32_t seg = (nbw + lanes - 1) / lanes, me = blockIdx.y * 256u + t;
    uint32_t lo = max(1u, me * seg), hi = min(nbw, (me + 1) * seg);
    Xyzz<F> run = xyzz_inf<F>(), acc = xyzz_inf<F>();
    for (uint32_t d = hi; d-- > lo;) {
        uint32_t b = (w << c) | d;
        if (off[b + 1] > off[b]) run = xyzz_add(run, part[off[b]]);
        acc = xyzz_add(acc, run);
    }
    if (lo < hi && lo > 1) acc = xyzz_add(acc, xyzz_mul_small(run, lo - 1));
    sh[t] = acc;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] = xyzz_add(sh[t], sh[t + s]);
        __syncthreads();
    }
    if (t == 0) wpart[w * gridDim.y + blockIdx.y] = sh[0];
}

// the gridDim.y partials of each window added by a tree: one workgroup per window, blockDim = that count (a power of two <= 256)
template <class F>
__global__ __launch_bounds__(256) void msm_window_sum_kernel(const Xyzz<F>* __restrict__ wpart, Xyzz<F>* __restrict__ win) {
    __shared__ Xyzz<F> sh[256];
    const uint32_t t = threadIdx.x, g = blockDim.x;
    sh[t] = wpart[blockIdx.x * g + t];
    __syncthreads();
    for (uint32_t s = g >> 1; s > 0; s >>= 1) {
        if (t < s) sh[t] = xyzz_add(sh[t], sh[t + s]);
        __syncthreads();
    }
    if (t == 0) win[blockIdx.x] = sh[0];
}

template <class F>
__global__ __launch_bounds__(256) void on_curve_kernel(const uint32_t* __restrict__ pts, size_t n, uint32_t* __restrict__ bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !on_curve(load_aff<F>(pts, i))) bad[0] = 1u;
}

// ---------------- Fr NTT ----------------
__device__ __forceinline__ Fr ld_fr(const uint32_t* p, size_t i) {
    Fr a;
    memcpy(&a, p + 8 * i, 32);
    return a;
}
__device__ __forceinline__ void st_fr(uint32_t* p, size_t i, const Fr& a) { memcpy(p + 8 * i, &a, 32); }

__global__ void twiddle_kernel(uint32_t* __restrict__ tw, uint32_t* __restrict__ itw, uint32_t half, Fr w, Fr wi) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= half) return;
    st_fr(tw, k, pow_u64(w, k, fr_one()));
    st_fr(itw, k, pow_u64(wi, k, fr_one()));
}

// one radix-2 stage over the whole array: butterflies (i, i + h), twiddle index j * (N / 2h)
template <bool DIF>
__global__ __launch_bounds__(256) void ntt_stage_kernel(uint32_t* __restrict__ x, const uint32_t* __restrict__ tw, uint32_t logN, uint32_t logh) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (1u << (logN - 1))) return;
    uint32_t h = 1u << logh, j = t & (h - 1);
    size_t i0 = ((size_t)(t >> logh) << (logh + 1)) | j, i1 = i0 + h;
    Fr w = ld_fr(tw, (size_t)j << (logN - 1 - logh));
    Fr a = ld_fr(x, i0), b = ld_fr(x, i1);
    if (DIF) {
        st_fr(x, i0, add(a, b));
        st_fr(x, i1, mul(sub(a, b), w));
    } else {
        b = mul(b, w);
        st_fr(x, i0, add(a, b));
        st_fr(x, i1, sub(a, b));
    }
}

// every stage with h < 2^logB inside one LDS block of 2^logB elements (DIF: h descending; DIT: ascending); blockDim = 2^(logB-1)
template <bool DIF>
__global__ __launch_bounds__(512) void ntt_lds_kernel(uint32_t* __restrict__ x, const uint32_t* __restrict__ tw, uint32_t logN, uint32_t logB) {
    __shared__ Fr s[1024];
    const uint32_t t = threadIdx.x, B = 1u << logB;
    const size_t base = (size_t)blockIdx.x << logB;
    s[t] = ld_fr(x, base + t);
    s[t + B / 2] = ld_fr(x, base + t + B / 2);
    __syncthreads();
    for (uint32_t k = 0; k < logB; k++) {
        uint32_t logh = DIF ? logB - 1 - k : k;
        uint32_t h = 1u << logh, j = t & (h - 1);
        uint32_t i0 = ((t >> logh) << (logh + 1)) | j, i1 = i0 + h;
        Fr w = ld_fr(tw, (size_t)j << (logN - 1 - logh));
        Fr a = s[i0], b = s[i1];
        if (DIF) {
            s[i0] = add(a, b);
            s[i1] = mul(sub(a, b), w);
        } else {
            b = mul(b, w);
            s[i0] = add(a, b);
            s[i1] = sub(a, b);
        }
        __syncthreads();
    }
    st_fr(x, base + t, s[t]);
    st_fr(x, base + t + B / 2, s[t + B / 2]);
}

// position p holds coefficient k = bitrev(p): times omega_2N^k / N = (k odd ? g : 1) * tw[k >> 1] / N
__global__ __launch_bounds__(256) void coset_scale_kernel(uint32_t* __restrict__ x, const uint32_t* __restrict__ tw, uint32_t logN, Fr ninv, Fr gninv) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (1u << logN)) return;
    uint32_t k = logN ? __brev(p) >> (32 - logN) : 0u;
    Fr f = mul((k & 1u) ? gninv : ninv, ld_fr(tw, k >> 1));
    st_fr(x, p, mul(ld_fr(x, p), f));
}

// ---------------- evaluation ----------------
// A_T, B_T at constraint c from the CSR lists (value c R^2 times canonical w = c w in Montgomery form), C_T = A_T B_T
__global__ __launch_bounds__(256) void eval_abc_kernel(const uint32_t* __restrict__ ra, const uint32_t* __restrict__ sa, const uint32_t* __restrict__ va,
                                                       const uint32_t* __restrict__ rb, const uint32_t* __restrict__ sb, const uint32_t* __restrict__ vb,
                                                       const uint32_t* __restrict__ wit, uint32_t N, uint32_t* __restrict__ poly) {
    uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    Fr a = fp_zero<FrP>(), b = fp_zero<FrP>();
    for (uint32_t e = ra[c]; e < ra[c + 1]; e++) a = add(a, mul(ld_fr(va, e), ld_fr(wit, sa[e])));
    for (uint32_t e = rb[c]; e < rb[c + 1]; e++) b = add(b, mul(ld_fr(vb, e), ld_fr(wit, sb[e])));
    st_fr(poly, c, a);
    st_fr(poly, (size_t)N + c, b);
    st_fr(poly, 2 * (size_t)N + c, mul(a, b));
}

// p_j = A B - C on the coset, canonical, into the C-MSM's scalars
__global__ __launch_bounds__(256) void eval_p_kernel(const uint32_t* __restrict__ poly, uint32_t N, uint32_t* __restrict__ out) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    Fr p = sub(mul(ld_fr(poly, j), ld_fr(poly, (size_t)N + j)), ld_fr(poly, 2 * (size_t)N + j));
    st_fr(out, j, from_mont(p));
}

inline unsigned grid(size_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

const char* scan_u32(bx_ctx* c, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* bsum) {
    uint32_t nblk = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (nblk) hipLaunchKernelGGL(scan_tile_kernel, dim3(nblk), dim3(256), 0, c->stream, in, out, bsum, n);
    hipLaunchKernelGGL(scan_bsum_kernel, dim3(1), dim3(256), 0, c->stream, bsum, nblk, out + n);
    if (n) hipLaunchKernelGGL(scan_add_kernel, dim3(grid(n, 256)), dim3(256), 0, c->stream, out, bsum, n);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}

uint32_t window_bits(size_t n) {
    int lg = bx::ilog2(n);
    return (uint32_t)std::min(16, std::max(4, lg - 4));
}

// scoped pool allocations of one call
struct Scratch {
    bx_ctx* c;
    std::vector<bx_buf> bufs;
    explicit Scratch(bx_ctx* ctx) : c(ctx) {}
    const char* get(size_t words, uint32_t** p) {
        bx_buf b{};
        BX_TRY(bx_alloc(c, words ? words : 1, &b));
        bufs.push_back(b);
        *p = (uint32_t*)b.dptr;
        return nullptr;
    }
    ~Scratch() {
        for (auto& b : bufs) (void)bx_release(c, b);
    }
};

// sum scalars[i] * pts[i], enqueued on the ctx's stream: win receives the W window sums S_w (XYZZ); the caller combines them as
// sum_w 2^(c w) S_w on the host (msm_entry).  *windows / *cbits: W and c.
template <class F>
const char* msm_run(bx_ctx* c, Scratch& s, const uint32_t* pts, const uint32_t* sc, size_t n, uint32_t** win, uint32_t* windows, uint32_t* cbits) {
    using X = Xyzz<F>;
    constexpr size_t XW = sizeof(X) / 4;
    const uint32_t cb = window_bits(n), W = (256 + cb - 1) / cb, nb = W << cb;
    BX_REQUIRE(c, n <= BX_BN254_MSM_MAX_N, "bn254 msm: n above BX_BN254_MSM_MAX_N");
    const uint32_t G = std::min(256u, std::max(1u, (1u << cb) / 2048u));  // workgroups per window in the weighted reduction
    uint32_t *cnt, *off, *sorted, *nch, *choff[2], *bsum, *part[2], *wpart;
    const size_t cap0 = (size_t)n * W / CHUNK + nb + 1, cap1 = cap0 / CHUNK + nb + 1;
    BX_TRY(s.get(nb, &cnt));
    BX_TRY(s.get(nb + 1, &off));
    BX_TRY(s.get((size_t)n * W, &sorted));
    BX_TRY(s.get(nb, &nch));
    BX_TRY(s.get(nb + 1, &choff[0]));
    BX_TRY(s.get(nb + 1, &choff[1]));
    BX_TRY(s.get(nb / SCAN_TILE + 2, &bsum));
    BX_TRY(s.get(cap0 * XW, &part[0]));
    BX_TRY(s.get(cap1 * XW, &part[1]));
    BX_TRY(s.get((size_t)W * G * XW, &wpart));
    BX_TRY(s.get((size_t)W * XW, win));
    hipStream_t st = c->stream;
    BX_HIP(c, hipMemsetAsync(cnt, 0, (size_t)nb * 4, st));
    hipLaunchKernelGGL((msm_bucket_kernel<F, false>), dim3(grid(n, 256)), dim3(256), 0, st, pts, sc, (uint32_t)n, cb, W, cnt, nullptr);
    BX_LAUNCH_CHECK(c);
    BX_TRY(scan_u32(c, cnt, off, nb, bsum));
    BX_HIP(c, hipMemcpyAsync(cnt, off, (size_t)nb * 4, hipMemcpyDeviceToDevice, st));  // cnt becomes the scatter cursors
    hipLaunchKernelGGL((msm_bucket_kernel<F, true>), dim3(grid(n, 256)), dim3(256), 0, st, pts, sc, (uint32_t)n, cb, W, cnt, sorted);
    BX_LAUNCH_CHECK(c);
    // level 0: chunks of the sorted index lists -> part[0]
    hipLaunchKernelGGL(msm_chunk_count_kernel, dim3(grid(nb, 256)), dim3(256), 0, st, off, nb, nch);
    BX_LAUNCH_CHECK(c);
    BX_TRY(scan_u32(c, nch, choff[0], nb, bsum));
    hipLaunchKernelGGL(msm_level0_kernel<F>, dim3(grid(cap0, 256)), dim3(256), 0, st, pts, sorted, off, choff[0], nb, (X*)part[0]);
    BX_LAUNCH_CHECK(c);
    // later levels until every bucket has one partial (a bucket holds at most n entries)
    int cur = 0;
    size_t bound = (n + CHUNK - 1) / CHUNK;
    while (bound > 1) {
        hipLaunchKernelGGL(msm_chunk_count_kernel, dim3(grid(nb, 256)), dim3(256), 0, st, choff[cur], nb, nch);
        BX_LAUNCH_CHECK(c);
        BX_TRY(scan_u32(c, nch, choff[cur ^ 1], nb, bsum));
        hipLaunchKernelGGL(msm_level_kernel<F>, dim3(grid(cur ? cap0 : cap1, 256)), dim3(256), 0, st, (const X*)part[cur], choff[cur], choff[cur ^ 1],
                           nb, (X*)part[cur ^ 1]);
        BX_LAUNCH_CHECK(c);
        cur ^= 1;
        bound = (bound + CHUNK - 1) / CHUNK;
    }
    hipLaunchKernelGGL(msm_window_reduce_kernel<F>, dim3(W, G), dim3(256), 0, st, (const X*)part[cur], choff[cur], cb, (X*)wpart);
    hipLaunchKernelGGL(msm_window_sum_kernel<F>, dim3(W), dim3(G), 0, st, (const X*)wpart, (X*)*win);
    BX_LAUNCH_CHECK(c);
    *windows = W;
    *cbits = cb;
    return nullptr;  // Scratch returns the buffers to the pool in stream order
}

template <class F>
const char* msm_entry(bx_ctx* c, bx_buf points, bx_buf scalars, size_t n, uint32_t* out, const char* name) {
    constexpr size_t PW = sizeof(Aff<F>) / 4;
    BX_REQUIRE(c, out != nullptr, "bn254 msm: null output");
    BX_REQUIRE(c, bx::mul_le(n, PW, points.len) && bx::mul_le(n, 8, scalars.len), "bn254 msm: buffer shorter than n points / scalars");
    BX_REQUIRE(c, n == 0 || (points.dptr && scalars.dptr), "bn254 msm: null buffer");
    if (n == 0) {
        memset(out, 0, PW * 4);
        return nullptr;
    }
    BX_ENTER(c);
    bx::OpScope op(c, name, (double)n * (PW + 8) * 4);
    uint32_t W = 0, cb = 0;
    {
        Scratch s(c);
        uint32_t* win;
        BX_TRY(msm_run<F>(c, s, (const uint32_t*)points.dptr, (const uint32_t*)scalars.dptr, n, &win, &W, &cb));
        BX_HIP(c, hipMemcpyAsync(c->h_stage, win, W * sizeof(Xyzz<F>), hipMemcpyDeviceToHost, c->stream));
    }
    BX_TRY(bx::sync_and_check_flag(c));
    // Horner over the W window sums and the affine conversion: c (W - 1) doublings, W additions, two inverses (host)
    std::vector<Xyzz<F>> ws(W);
    memcpy(ws.data(), c->h_stage, W * sizeof(Xyzz<F>));
    Xyzz<F> acc = ws[W - 1];
    for (int w = (int)W - 2; w >= 0; w--) {
        for (uint32_t k = 0; k < cb; k++) acc = xyzz_dbl(acc);
        acc = xyzz_add(acc, ws[w]);
    }
    Aff<F> a = to_affine_canonical(acc);
    memcpy(out, &a, PW * 4);
    return nullptr;
}

// ---------------- key ----------------
const char* key_alloc(bx_ctx* c, bx_groth16_key* k, size_t words, uint32_t** p) {
    void* d = nullptr;
    BX_HIP(c, hipMalloc(&d, (words ? words : 1) * 4));
    k->allocs.push_back(d);
    *p = (uint32_t*)d;
    return nullptr;
}

void key_release(bx_groth16_key* k) {
    for (void* p : k->allocs) (void)hipFree(p);
    k->allocs.clear();
    if (k->h_pin) (void)hipHostFree(k->h_pin);
    k->h_pin = nullptr;
}

// host -> device through a pinned staging buffer (the key's, allocated once): chunks are copied into it back to back and uploaded
// without a wait; the stream is drained only before the buffer is reused.  One Stager per sequence of uploads that starts with the
// stream drained (key load, a proof).
struct Stager {
    bx_ctx* c;
    uint8_t* pin;
    size_t cap, used = 0;
    Stager(bx_ctx* ctx, bx_groth16_key* k) : c(ctx), pin((uint8_t*)k->h_pin), cap(k->pin_bytes) {}
    const char* put(void* dst, const void* src, size_t bytes) {
        for (size_t o = 0; o < bytes;) {
            if (used == cap) {
                BX_HIP(c, bx::stream_wait(c));
                used = 0;
            }
            size_t m = std::min(cap - used, bytes - o);
            memcpy(pin + used, (const uint8_t*)src + o, m);
            BX_HIP(c, hipMemcpyAsync((uint8_t*)dst + o, pin + used, m, hipMemcpyHostToDevice, c->stream));
            used += m;
            o += m;
        }
        return nullptr;
    }
};

Fr fr_words(const uint32_t* w) {
    Fr a;
    memcpy(a.v, w, 32);
    return a;
}

const char* ntt_coset(bx_ctx* c, bx_groth16_key* k, uint32_t* x) {
    const uint32_t N = k->info.domain_size, logN = (uint32_t)bx::ilog2(N), logB = std::min(logN, 10u);
    hipStream_t st = c->stream;
    // inverse, decimation in frequency: global stages h >= 2^logB, then the rest in LDS
    for (uint32_t logh = logN; logh-- > logB;)
        hipLaunchKernelGGL(ntt_stage_kernel<true>, dim3(grid(N / 2, 256)), dim3(256), 0, st, x, k->d_itw, logN, logh);
    if (logB) hipLaunchKernelGGL(ntt_lds_kernel<true>, dim3(N >> logB), dim3(1u << (logB - 1)), 0, st, x, k->d_itw, logN, logB);
    Fr ninv = fr_words(k->ninv_mont), gninv = mul(fr_words(k->omega2n_mont), ninv);
    hipLaunchKernelGGL(coset_scale_kernel, dim3(grid(N, 256)), dim3(256), 0, st, x, k->d_tw, logN, ninv, gninv);
    // forward, decimation in time: LDS stages first, then h >= 2^logB
    if (logB) hipLaunchKernelGGL(ntt_lds_kernel<false>, dim3(N >> logB), dim3(1u << (logB - 1)), 0, st, x, k->d_tw, logN, logB);
    for (uint32_t logh = logB; logh < logN; logh++)
        hipLaunchKernelGGL(ntt_stage_kernel<false>, dim3(grid(N / 2, 256)), dim3(256), 0, st, x, k->d_tw, logN, logh);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}

// Every coordinate of `count` points (`coords` 32-byte Fq limbs each) is below q.  Host only, over the zkey's bytes: the field code
// assumes reduced inputs (its equality and zero tests are limb compares), so an encoding x + q of a coordinate can pass on_curve and
// then miss the doubling branch of an addition — a wrong sum that comes back fully reduced.
const char* coords_below_q(bx_ctx* c, const uint8_t* p, size_t count, size_t coords, const char* what) {
    for (size_t i = 0; i < count * coords; i++) {
        uint32_t w[8];
        memcpy(w, p + 32 * i, 32);
        if (ge_mod<FqP>(w)) {
            snprintf(c->err, sizeof c->err, "bx_groth16_key_load: %s: point %zu has a coordinate not below q", what, i / coords);
            return c->err;
        }
    }
    return nullptr;
}

const char* key_load(bx_ctx* c, const uint8_t* p, size_t len, bx_groth16_key* k) {
    bx::ZkeyView z;
    char msg[256];
    if (bx::zkey_parse(p, len, &z, msg, sizeof msg)) return bx::set_msg(c, msg);
    const bx_groth16_info& I = z.info;
    BX_REQUIRE(c, I.n_public <= BX_GROTH16_MAX_PUBLIC, "bx_groth16_key_load: more public signals than BX_GROTH16_MAX_PUBLIC");
    k->info = I;
    const size_t n = I.n_vars, N = I.domain_size, nc = I.n_vars - I.n_public - 1, half = std::max<size_t>(1, N / 2);
    BX_REQUIRE(c, n + 2 <= BX_BN254_MSM_MAX_N && nc + N + 3 <= BX_BN254_MSM_MAX_N,
               "bx_groth16_key_load: the key's MSMs (n_vars + 2, n_vars - n_public - 1 + domain_size + 3 points) exceed BX_BN254_MSM_MAX_N");
    // coordinates below q, over the bytes about to be staged (and IC / gamma2, which stay on the host)
    {
        const uint8_t* h = z.sec[2];
        const struct {
            const uint8_t* at;
            size_t count, coords;
            const char* what;
        } lists[] = {{h + 84, 1, 2, "section 2 (alpha1)"}, {h + 148, 1, 2, "section 2 (beta1)"},  {h + 212, 1, 4, "section 2 (beta2)"},
                     {h + 340, 1, 4, "section 2 (gamma2)"}, {h + 468, 1, 2, "section 2 (delta1)"}, {h + 532, 1, 4, "section 2 (delta2)"},
                     {z.sec[3], (size_t)I.n_public + 1, 2, "section 3 (IC)"}, {z.sec[5], n, 2, "section 5 (A)"}, {z.sec[6], n, 2, "section 6 (B1)"},
                     {z.sec[7], n, 4, "section 7 (B2)"}, {z.sec[8], nc, 2, "section 8 (C)"}, {z.sec[9], N, 2, "section 9 (H)"}};
        for (auto& l : lists) BX_TRY(coords_below_q(c, l.at, l.count, l.coords, l.what));
    }
    // IC and gamma2 take no part in proving (they are uploaded nowhere): checked here, on the host
    for (uint32_t i = 0; i <= I.n_public; i++) {
        Aff<Fq> p;
        memcpy(&p, z.sec[3] + 64 * (size_t)i, 64);
        BX_REQUIRE(c, on_curve(p), "bx_groth16_key_load: an IC point is not on its curve (endianness or Montgomery form?)");
    }
    {
        Aff<Fq2> g;
        memcpy(&g, z.sec[2] + 340, 128);
        BX_REQUIRE(c, on_curve(g), "bx_groth16_key_load: gamma2 is not on its curve (endianness or Montgomery form?)");
    }
    k->vk_header.assign(z.sec[2], z.sec[2] + z.sec_len[2]);
    k->vk_ic.assign(z.sec[3], z.sec[3] + z.sec_len[3]);
    k->pin_bytes = std::min<size_t>((size_t)64 << 20, len + 4096);
    BX_HIP(c, hipHostMalloc(&k->h_pin, k->pin_bytes, hipHostMallocDefault));
    k->n_c = (uint32_t)nc;
    const uint8_t* s2 = z.sec[2];
    const uint8_t *alpha1 = s2 + 84, *beta1 = s2 + 148, *beta2 = s2 + 212, *delta1 = s2 + 468, *delta2 = s2 + 532;
    BX_TRY(key_alloc(c, k, (n + 2) * 16, &k->d_a));
    BX_TRY(key_alloc(c, k, (n + 2) * 16, &k->d_b1));
    BX_TRY(key_alloc(c, k, (n + 2) * 32, &k->d_b2));
    BX_TRY(key_alloc(c, k, (nc + N + 3) * 16, &k->d_ch));
    BX_TRY(key_alloc(c, k, half * 8, &k->d_tw));
    BX_TRY(key_alloc(c, k, half * 8, &k->d_itw));
    BX_TRY(key_alloc(c, k, (n + 2) * 8, &k->d_sa));
    BX_TRY(key_alloc(c, k, (n + 2) * 8, &k->d_sb));
    BX_TRY(key_alloc(c, k, (nc + N + 3) * 8, &k->d_sc));
    BX_TRY(key_alloc(c, k, 3 * N * 8, &k->d_poly));
    Stager up(c, k);
    BX_TRY(up.put(k->d_a, z.sec[5], n * 64));
    BX_TRY(up.put(k->d_a + n * 16, alpha1, 64));
    BX_TRY(up.put(k->d_a + (n + 1) * 16, delta1, 64));
    BX_TRY(up.put(k->d_b1, z.sec[6], n * 64));
    BX_TRY(up.put(k->d_b1 + n * 16, beta1, 64));
    BX_TRY(up.put(k->d_b1 + (n + 1) * 16, delta1, 64));
    BX_TRY(up.put(k->d_b2, z.sec[7], n * 128));
    BX_TRY(up.put(k->d_b2 + n * 32, beta2, 128));
    BX_TRY(up.put(k->d_b2 + (n + 1) * 32, delta2, 128));
    BX_TRY(up.put(k->d_ch, z.sec[8], nc * 64));
    BX_TRY(up.put(k->d_ch + nc * 16, z.sec[9], N * 64));
    BX_HIP(c, hipMemsetAsync(k->d_ch + (nc + N) * 16, 0, 2 * 64, c->stream));
    BX_TRY(up.put(k->d_ch + (nc + N + 2) * 16, delta1, 64));
    // coefficient lists by constraint (CSR), A (matrix 0) and B (matrix 1)
    const uint8_t* s4 = z.sec[4];
    const uint64_t ncoef = I.n_coefs;
    for (int m = 0; m < 2; m++) {
        std::vector<uint32_t> rows(N + 1, 0);
        for (uint64_t e = 0; e < ncoef; e++) {
            uint32_t rec[3];
            memcpy(rec, s4 + 4 + e * 44, 12);
            if (rec[0] == (uint32_t)m) rows[rec[1] + 1]++;
        }
        for (size_t i = 0; i < N; i++) rows[i + 1] += rows[i];
        const size_t cnt = rows[N];
        std::vector<uint32_t> sig(std::max<size_t>(cnt, 1)), val(std::max<size_t>(cnt, 1) * 8), cur(rows.begin(), rows.end() - 1);
        for (uint64_t e = 0; e < ncoef; e++) {
            uint32_t rec[3];
            memcpy(rec, s4 + 4 + e * 44, 12);
            if (rec[0] != (uint32_t)m) continue;
            uint32_t at = cur[rec[1]]++;
            sig[at] = rec[2];
            memcpy(&val[(size_t)at * 8], s4 + 4 + e * 44 + 12, 32);
        }
        BX_TRY(key_alloc(c, k, N + 1, &k->d_rows[m]));
        BX_TRY(key_alloc(c, k, sig.size(), &k->d_sig[m]));
        BX_TRY(key_alloc(c, k, val.size(), &k->d_val[m]));
        BX_TRY(up.put(k->d_rows[m], rows.data(), rows.size() * 4));
        BX_TRY(up.put(k->d_sig[m], sig.data(), sig.size() * 4));
        BX_TRY(up.put(k->d_val[m], val.data(), val.size() * 4));
    }
    // twiddles: omega_N = omega_2^28 squared (28 - logN) times; omega_2N one squaring less
    const int logN = bx::ilog2(N);
    Fr w2n = fr_root28(), wi2n = fr_root28_inv();
    for (int i = 0; i < 27 - logN; i++) {
        w2n = sqr(w2n);
        wi2n = sqr(wi2n);
    }
    Fr wn = sqr(w2n), win = sqr(wi2n);
    memcpy(k->omega2n_mont, w2n.v, 32);
    Fr nm = to_mont(fp_from<FrP>({(uint32_t)N, 0, 0, 0, 0, 0, 0, 0}));
    Fr ni = inv(nm);
    memcpy(k->ninv_mont, ni.v, 32);
    hipLaunchKernelGGL(twiddle_kernel, dim3(grid(half, 256)), dim3(256), 0, c->stream, k->d_tw, k->d_itw, (uint32_t)half, wn, win);
    BX_LAUNCH_CHECK(c);
    // every point on its curve (the A / B1 slots of CH are zeros = infinity until a proof writes them)
    uint32_t* bad;
    BX_TRY(key_alloc(c, k, 1, &bad));
    BX_HIP(c, hipMemsetAsync(bad, 0, 4, c->stream));
    hipLaunchKernelGGL(on_curve_kernel<Fq>, dim3(grid(n + 2, 256)), dim3(256), 0, c->stream, k->d_a, n + 2, bad);
    hipLaunchKernelGGL(on_curve_kernel<Fq>, dim3(grid(n + 2, 256)), dim3(256), 0, c->stream, k->d_b1, n + 2, bad);
    hipLaunchKernelGGL(on_curve_kernel<Fq2>, dim3(grid(n + 2, 256)), dim3(256), 0, c->stream, k->d_b2, n + 2, bad);
    hipLaunchKernelGGL(on_curve_kernel<Fq>, dim3(grid(nc + N + 3, 256)), dim3(256), 0, c->stream, k->d_ch, nc + N + 3, bad);
    BX_LAUNCH_CHECK(c);
    uint32_t hbad = 0;
    BX_HIP(c, hipMemcpyAsync(&hbad, bad, 4, hipMemcpyDeviceToHost, c->stream));
    BX_HIP(c, bx::stream_wait(c));
    BX_REQUIRE(c, hbad == 0, "bx_groth16_key_load: a key point is not on its curve (endianness or Montgomery form?)");
    return nullptr;
}

// the keys loaded on each ctx, so that bx_free releases the ones its caller did not
std::mutex g_keys_mu;
std::map<bx_ctx*, std::set<bx_groth16_key*>> g_keys;

bool rand_fr(uint32_t out[8]) {
    for (int tries = 0; tries < 64; tries++) {
        size_t got = 0;
        while (got < 32) {
            ssize_t r = getrandom((uint8_t*)out + got, 32 - got, 0);
            if (r <= 0) return false;
            got += (size_t)r;
        }
        out[7] &= 0x3FFFFFFFu;  // below 2^254; reject >= r
        if (!ge_mod<FrP>(out)) return true;
    }
    return false;
}

}  // namespace

extern "C" const char* bx_bn254_msm_g1(bx_ctx* c, bx_buf points, bx_buf scalars, size_t n, uint32_t* out) try {
    if (!c) return "bx_bn254_msm_g1: null ctx";
    return msm_entry<Fq>(c, points, scalars, n, out, "bn254_msm_g1");
} BX_ABI_CATCH(c, "bx_bn254_msm_g1")

extern "C" const char* bx_bn254_msm_g2(bx_ctx* c, bx_buf points, bx_buf scalars, size_t n, uint32_t* out) try {
    if (!c) return "bx_bn254_msm_g2: null ctx";
    return msm_entry<Fq2>(c, points, scalars, n, out, "bn254_msm_g2");
} BX_ABI_CATCH(c, "bx_bn254_msm_g2")

extern "C" const char* bx_groth16_key_load_mem(bx_ctx* c, const void* bytes, size_t len, bx_groth16_key** out) try {
    if (!c) return "bx_groth16_key_load: null ctx";
    BX_REQUIRE(c, out != nullptr && (bytes != nullptr || len == 0), "bx_groth16_key_load: null argument");
    *out = nullptr;
    BX_ENTER(c);
    bx_groth16_key* k = new bx_groth16_key;
    k->ctx = c;
    const char* m = key_load(c, (const uint8_t*)bytes, len, k);
    if (m) {
        (void)bx::stream_wait(c);
        key_release(k);
        delete k;
        return m;
    }
    {
        std::lock_guard<std::mutex> g(g_keys_mu);
        g_keys[c].insert(k);
    }
    *out = k;
    return nullptr;
} BX_ABI_CATCH(c, "bx_groth16_key_load")

extern "C" const char* bx_groth16_key_load(bx_ctx* c, const char* path, bx_groth16_key** out) try {
    if (!c) return "bx_groth16_key_load: null ctx";
    BX_REQUIRE(c, path != nullptr && out != nullptr, "bx_groth16_key_load: null argument");
    FILE* f = fopen(path, "rb");
    if (!f) {
        snprintf(c->err, sizeof c->err, "bx_groth16_key_load: cannot open %s", path);
        return c->err;
    }
    std::vector<uint8_t> data;
    if (fseek(f, 0, SEEK_END) == 0) {
        long sz = ftell(f);
        if (sz > 0) data.resize((size_t)sz);
        rewind(f);
    }
    size_t got = data.empty() ? 0 : fread(data.data(), 1, data.size(), f);
    fclose(f);
    data.resize(got);
    return bx_groth16_key_load_mem(c, data.data(), data.size(), out);
} BX_ABI_CATCH(c, "bx_groth16_key_load")

extern "C" const char* bx_groth16_key_info(const bx_groth16_key* k, bx_groth16_info* out) {
    if (!k || !out) return "bx_groth16_key_info: null argument";
    *out = k->info;
    return nullptr;
}

extern "C" const char* bx_groth16_key_free(bx_ctx* c, bx_groth16_key* k) try {
    if (!c) return "bx_groth16_key_free: null ctx";
    if (!k) return nullptr;
    BX_REQUIRE(c, k->ctx == c, "bx_groth16_key_free: the key belongs to another ctx");
    BX_ENTER(c);
    BX_HIP(c, bx::stream_wait(c));
    {
        std::lock_guard<std::mutex> g(g_keys_mu);
        auto it = g_keys.find(c);
        if (it != g_keys.end()) {
            it->second.erase(k);
            if (it->second.empty()) g_keys.erase(it);
        }
    }
    key_release(k);
    delete k;
    return nullptr;
} BX_ABI_CATCH(c, "bx_groth16_key_free")

namespace bx {
void groth16_release_keys(bx_ctx* c) {
    std::set<bx_groth16_key*> ks;
    {
        std::lock_guard<std::mutex> g(g_keys_mu);
        auto it = g_keys.find(c);
        if (it == g_keys.end()) return;
        ks.swap(it->second);
        g_keys.erase(it);
    }
    (void)hipSetDevice(c->device);
    (void)bx::stream_wait(c);
    for (bx_groth16_key* k : ks) {
        key_release(k);
        delete k;
    }
}
}  // namespace bx

extern "C" const char* bx_groth16_prove(bx_ctx* c, bx_groth16_key* k, const void* witness, size_t n_vars, const void* rs, bx_groth16_proof* out) try {
    if (!c) return "bx_groth16_prove: null ctx";
    BX_REQUIRE(c, k != nullptr && witness != nullptr && out != nullptr, "bx_groth16_prove: null argument");
    BX_REQUIRE(c, k->ctx == c, "bx_groth16_prove: the key belongs to another ctx");
    const bx_groth16_info& I = k->info;
    BX_REQUIRE(c, n_vars == I.n_vars, "bx_groth16_prove: witness length does not match the key's n_vars");
    const uint32_t* w = (const uint32_t*)witness;
    for (size_t i = 0; i < n_vars; i++)
        if (ge_mod<FrP>(w + 8 * i)) {
            snprintf(c->err, sizeof c->err, "bx_groth16_prove: witness[%zu] is not below r", i);
            return c->err;
        }
    BX_REQUIRE(c, w[0] == 1 && !(w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]), "bx_groth16_prove: witness[0] must be 1");
    uint32_t r[8], s[8];
    if (rs) {
        memcpy(r, rs, 32);
        memcpy(s, (const uint8_t*)rs + 32, 32);
        BX_REQUIRE(c, !ge_mod<FrP>(r) && !ge_mod<FrP>(s), "bx_groth16_prove: r or s is not below r");
    } else {
        BX_REQUIRE(c, rand_fr(r) && rand_fr(s), "bx_groth16_prove: no OS randomness");
    }
    BX_ENTER(c);
    const size_t n = n_vars, N = I.domain_size, nc = k->n_c, npub = I.n_public;
    hipStream_t st = c->stream;
    {
        bx::OpScope op(c, "groth16_upload", (double)n * 32);
        Stager up(c, k);
        BX_TRY(up.put(k->d_sa, w, n * 32));
        uint32_t extra_a[16] = {1, 0, 0, 0, 0, 0, 0, 0}, extra_b[16] = {1, 0, 0, 0, 0, 0, 0, 0};
        memcpy(extra_a + 8, r, 32);
        memcpy(extra_b + 8, s, 32);
        BX_TRY(up.put(k->d_sa + n * 8, extra_a, 64));
        BX_HIP(c, hipMemcpyAsync(k->d_sb, k->d_sa, n * 32, hipMemcpyDeviceToDevice, st));
        BX_TRY(up.put(k->d_sb + n * 8, extra_b, 64));
        if (nc) BX_HIP(c, hipMemcpyAsync(k->d_sc, k->d_sa + (npub + 1) * 8, nc * 32, hipMemcpyDeviceToDevice, st));
        // s, r, -r s
        Fr rm = to_mont(fr_words(r)), sm = to_mont(fr_words(s));
        Fr nrs = from_mont(neg(mul(rm, sm)));
        uint32_t extra_c[24];
        memcpy(extra_c, s, 32);
        memcpy(extra_c + 8, r, 32);
        memcpy(extra_c + 16, nrs.v, 32);
        BX_TRY(up.put(k->d_sc + (nc + N) * 8, extra_c, 96));
    }
    {
        bx::OpScope op(c, "groth16_eval", (double)N * 96);
        hipLaunchKernelGGL(eval_abc_kernel, dim3(grid(N, 256)), dim3(256), 0, st, k->d_rows[0], k->d_sig[0], k->d_val[0], k->d_rows[1], k->d_sig[1],
                           k->d_val[1], k->d_sa, (uint32_t)N, k->d_poly);
        BX_LAUNCH_CHECK(c);
    }
    {
        bx::OpScope op(c, "groth16_ntt", (double)N * 96 * 2);
        for (int m = 0; m < 3; m++) BX_TRY(ntt_coset(c, k, k->d_poly + (size_t)m * N * 8));
        hipLaunchKernelGGL(eval_p_kernel, dim3(grid(N, 256)), dim3(256), 0, st, k->d_poly, (uint32_t)N, k->d_sc + nc * 8);
        BX_LAUNCH_CHECK(c);
    }
    uint32_t a[16], b1[16];
    BX_TRY(bx_bn254_msm_g1(c, bx_buf{k->d_a, (n + 2) * 16}, bx_buf{k->d_sa, (n + 2) * 8}, n + 2, a));
    BX_TRY(bx_bn254_msm_g2(c, bx_buf{k->d_b2, (n + 2) * 32}, bx_buf{k->d_sb, (n + 2) * 8}, n + 2, out->b));
    BX_TRY(bx_bn254_msm_g1(c, bx_buf{k->d_b1, (n + 2) * 16}, bx_buf{k->d_sb, (n + 2) * 8}, n + 2, b1));
    // A and B1 into the C-MSM's point slots, Montgomery form (infinity stays zeros)
    uint32_t ab[32];
    for (int i = 0; i < 4; i++) {
        Fq v;
        memcpy(v.v, (i < 2 ? a : b1) + 8 * (i & 1), 32);
        v = to_mont(v);
        memcpy(ab + 8 * i, v.v, 32);
    }
    {
        Stager up(c, k);
        BX_TRY(up.put(k->d_ch + (nc + N) * 16, ab, sizeof ab));
    }
    BX_TRY(bx_bn254_msm_g1(c, bx_buf{k->d_ch, (nc + N + 3) * 16}, bx_buf{k->d_sc, (nc + N + 3) * 8}, nc + N + 3, out->c));
    memcpy(out->a, a, sizeof a);
    out->n_public = (uint32_t)npub;
    memset(out->public_signals, 0, sizeof out->public_signals);
    memcpy(out->public_signals, w + 8, npub * 32);
    return nullptr;
} BX_ABI_CATCH(c, "bx_groth16_prove")
