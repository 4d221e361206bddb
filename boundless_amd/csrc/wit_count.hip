// wit_count.hip — the multiplicity columns of a witness program ("multiplicity columns" of include/bx_program.h is the normative text): a
// general device histogram over whole data columns, run by bx_wit_program_run after the per-row program.  A translation unit of its
// own, so that wit_program_kernel's code object does not change.
//   input     directly the source columns of `data`, rows [0, rows): no gathered copy.  The work is cut into TILES of one workgroup's
//             width of consecutive rows of ONE source column; a workgroup takes a run of consecutive tiles.  The source index is
//             therefore wave-uniform (it comes from the uploaded table through the scalar cache, the column offset is
//             (size_t)col << po2), a wave reads 256 consecutive bytes, and every lane of a workgroup makes the same number of
//             trips: whole waves reach the ballots.  A lane whose row is at or past `rows` reads nothing and holds "no value".
//   waves     the lanes that hit the first live lane's bin are counted with one ballot and added by one lane, the rest add 1 each
//             (lookup_hist_lds_kernel's scheme, lookup.hip): a constant column costs one atomic per wave, not 64 on one address
//   LDS form  B <= 32 768 bins (128 KiB of the CU's 160): per-workgroup bins in dynamic LDS, 1024 lanes; every non-zero bin is flushed
//             with one global atomic
//   global    above that, or with the ctx tunable lookup_hist_lds = 0: the same loop with the atomics on the global bins, 256 lanes
//   store     data[col][r] = the Montgomery word of counts[r] below B, 0 from B to rows; rows at or above `rows` are not touched
// A count is at most 64 sources x 2^24 rows = 2^30 < P: a bin never wraps and its word needs no reduction.
// No inline assembly, nothing per lane in an array indexed at run time.
#include <vector>

#include "wit_program_dev.hpp"

namespace bx {

constexpr uint32_t WC_LDS_T = 1024, WC_GLOBAL_T = 256;
constexpr uint32_t WC_LDS_MAX_BINS = 32768;  // 128 KiB

// the geometry of one histogram launch: tiles of T rows, n_tiles = n_sources * tiles_per_col of them, tiles_per_wg per workgroup
struct WcRun {
    uint32_t po2, rows, bins, tiles_per_col, n_tiles, tiles_per_wg;
};

// one value per lane (v >= B: none) into `bins`; called by whole waves
__device__ __forceinline__ void wc_add(uint32_t* bins, uint32_t v, uint32_t B, uint32_t lane) {
    const bool live = v < B;
    const uint64_t any = __ballot(live);
    if (!any) return;
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)any) - 1;
    const uint32_t lb = __shfl(v, (int)leader);
    const bool peer = live && v == lb;
    const uint64_t peers = __ballot(peer);
    if (lane == leader) atomicAdd(&bins[lb], (uint32_t)__popcll(peers));
    else if (live && !peer) atomicAdd(&bins[v], 1u);
}

// the tiles of this workgroup, T rows each, into `bins`
template <uint32_t T>
__device__ __forceinline__ void wc_tiles(uint32_t* bins, const uint32_t* __restrict__ data, const uint32_t* __restrict__ sources, const WcRun& g) {
    const uint32_t t0 = blockIdx.x * g.tiles_per_wg;
    const uint32_t t1 = g.n_tiles - t0 < g.tiles_per_wg ? g.n_tiles : t0 + g.tiles_per_wg;  // the launch has t0 < n_tiles
    uint32_t q = t0 / g.tiles_per_col, c = t0 - q * g.tiles_per_col;  // source index and tile within its column: workgroup-uniform
    const uint32_t lane = __lane_id();
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t* col = data + ((size_t)sources[q] << g.po2);
        const uint32_t j = c * T + threadIdx.x;
        uint32_t v = g.bins;
        if (j < g.rows) v = fp_decode(col[j]);
        wc_add(bins, v, g.bins, lane);
        if (++c == g.tiles_per_col) {
            c = 0;
            ++q;
        }
    }
}

__global__ __launch_bounds__(WC_LDS_T) void wit_count_lds_kernel(uint32_t* __restrict__ counts, const uint32_t* __restrict__ data,
                                                                 const uint32_t* __restrict__ sources, WcRun g) {
    extern __shared__ uint32_t wc_bins[];  // g.bins words
    for (uint32_t b = threadIdx.x; b < g.bins; b += WC_LDS_T) wc_bins[b] = 0u;
    __syncthreads();
    wc_tiles<WC_LDS_T>(wc_bins, data, sources, g);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < g.bins; b += WC_LDS_T) {
        const uint32_t cnt = wc_bins[b];
        if (cnt) atomicAdd(&counts[b], cnt);
    }
}

__global__ __launch_bounds__(WC_GLOBAL_T) void wit_count_global_kernel(uint32_t* counts, const uint32_t* __restrict__ data,
                                                                       const uint32_t* __restrict__ sources, WcRun g) {
    wc_tiles<WC_GLOBAL_T>(counts, data, sources, g);
}

__global__ __launch_bounds__(256) void wit_count_store_kernel(uint32_t* __restrict__ col, const uint32_t* __restrict__ counts, uint32_t rows, uint32_t bins) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= rows) return;
    col[r] = r < bins ? fp_mul(R2, counts[r]) : 0u;
}

const char* wit_counts_load(bx_ctx* c, bx_wit_program_dev* d, const bx_wit_program* prog) {
    d->counts = prog->counts;
    if (d->counts.empty()) return nullptr;
    size_t total_bins = 0, lds_words = 0;
    for (const WitCount& ct : d->counts) {
        d->count_src_off.push_back(d->count_flat.size());
        d->count_bin_off.push_back(total_bins);
        d->count_flat.insert(d->count_flat.end(), ct.sources.begin(), ct.sources.end());
        total_bins += ct.bins;
        if (ct.bins <= WC_LDS_MAX_BINS && ct.bins > lds_words) lds_words = ct.bins;
    }
    BX_TRY(d->count_sources.alloc(c, d->count_flat.size()));
    BX_TRY(d->count_bins.alloc(c, total_bins));
    // a table of 2^15 bins needs more dynamic LDS than a kernel may use by default (set once per process and kernel; cheap to repeat)
    BX_REQUIRE(c, lds_words * 4 <= 64 * 1024 ||
                      hipFuncSetAttribute((const void*)wit_count_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(WC_LDS_MAX_BINS * 4)) == hipSuccess,
               "bx_wit_program_load: the count histogram's LDS bins could not be reserved");
    // the caller waits for the stream before count_flat can go away (it lives as long as the loaded program anyway)
    BX_HIP(c, hipMemcpyAsync(d->count_sources.b.dptr, d->count_flat.data(), d->count_flat.size() * 4, hipMemcpyHostToDevice, c->stream));
    return nullptr;
}

const char* wit_counts_run(bx_ctx* c, bx_wit_program_dev* d, uint32_t po2, bx_buf data) {
    const uint32_t n = 1u << po2;
    for (size_t k = 0; k < d->counts.size(); ++k) {  // the caller has checked every count against N and w_data
        const WitCount& ct = d->counts[k];
        const uint32_t rows = ct.rows ? ct.rows : n, n_src = (uint32_t)ct.sources.size();
        uint32_t* bins = (uint32_t*)d->count_bins.b.dptr + d->count_bin_off[k];
        const uint32_t* sources = (const uint32_t*)d->count_sources.b.dptr + d->count_src_off[k];
        BX_HIP(c, hipMemsetAsync(bins, 0, (size_t)ct.bins * 4, c->stream));
        {
            const bool lds = c->lookup_hist_lds && ct.bins <= WC_LDS_MAX_BINS;
            const uint32_t T = lds ? WC_LDS_T : WC_GLOBAL_T;
            WcRun g;
            g.po2 = po2, g.rows = rows, g.bins = ct.bins;
            g.tiles_per_col = (rows + T - 1) / T;
            g.n_tiles = n_src * g.tiles_per_col;  // at most 64 * 2^24 / 256 = 2^22
            // at least 8 tiles per workgroup; the LDS form one workgroup per CU (a 128 KiB table leaves room for no second one)
            const uint32_t max_wgs = lds ? (uint32_t)c->cu_count : 8u * (uint32_t)c->cu_count;
            uint32_t wgs = (g.n_tiles + 7) / 8;
            if (wgs > max_wgs) wgs = max_wgs;
            g.tiles_per_wg = (g.n_tiles + wgs - 1) / wgs;
            wgs = (g.n_tiles + g.tiles_per_wg - 1) / g.tiles_per_wg;  // no workgroup without a tile
            OpScope op(c, "wit_program_count", 4.0 * (double)rows * (double)n_src);  // the histogram kernel alone
            if (lds)
                hipLaunchKernelGGL(wit_count_lds_kernel, dim3(wgs), dim3(WC_LDS_T), (size_t)ct.bins * 4, c->stream, bins, (const uint32_t*)data.dptr, sources, g);
            else
                hipLaunchKernelGGL(wit_count_global_kernel, dim3(wgs), dim3(WC_GLOBAL_T), 0, c->stream, bins, (const uint32_t*)data.dptr, sources, g);
            BX_LAUNCH_CHECK(c);
        }
        OpScope op(c, "wit_program_count_store", 4.0 * ((double)rows + (double)(ct.bins < rows ? ct.bins : rows)));
        hipLaunchKernelGGL(wit_count_store_kernel, dim3((rows + 255) / 256), dim3(256), 0, c->stream, (uint32_t*)data.dptr + ((size_t)ct.col << po2),
                           (const uint32_t*)bins, rows, ct.bins);
        BX_LAUNCH_CHECK(c);
    }
    return nullptr;
}

}  // namespace bx
