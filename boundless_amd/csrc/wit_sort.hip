// wit_sort.hip — the sorted columns of a witness program ("sorted columns" of include/bx_program.h is the normative text): a stable LSD
// radix sort of whole data columns on the device, run by bx_wit_program_run after the per-row program and before the counts.  A
// translation unit of its own, so that no existing kernel's code object changes.
//   pack      the key columns are decoded ONCE into one uint64_t composite key per row, most significant key in the high bits (the bits
//             of a sort sum to at most 64), with idx[r] = r.  The passes move (key, idx) pairs, kept as two arrays: a wave reads 512 +
//             256 consecutive bytes.  Bits above the sum are zero, so a last pass with fewer than 8 live bits needs no special case.
//   passes    ceil(sum of bits / 8) passes of 8-bit digits, least significant first, ping-pong between two pair buffers.  The rows are
//             cut into TILES of WS_TILE = 1024 consecutive rows: 256 lanes x 4 trips, row = tile * 1024 + trip * 256 + wave * 64 + lane,
//             so row order within a tile is (trip, wave, lane) order.  A workgroup takes a run of consecutive tiles (at least two when
//             there are that many); every lane makes every trip, so whole waves reach the ballots, and a lane whose row is at or past
//             `rows` holds no element.
//     hist      per tile 256 LDS bins; the lanes of a wave with equal digits are found with a ballot per digit bit (ws_match) and
//               counted by the lowest of them: an all-equal column costs one LDS atomic per wave and trip, not 64 on one address.
//               Written digit-major, table[digit][tile]: the exclusive scan of the table in memory order is then exactly where each
//               tile's run of each digit starts in the output.
//     scan      two launches over the 256 * n_tiles words, in chunks of WS_CHUNK = 2048 (8 per lane, two 16-byte loads): the chunk sums,
//               then per chunk the sum of the chunks before it (at most 2048 words re-read per workgroup: no third launch, no
//               cross-workgroup waiting) and the exclusive scan in place.  scan.hip's u32 scan is not reused: a new instantiation
//               there would change its code object.
//     scatter   the workgroup re-reads its tile.  rank within the wave = the peers below the lane (ws_match again); across waves and
//               trips: per trip every wave leaves its digit counts in LDS (wcnt[wave][digit]), a lane adds the counts of the waves
//               before its own to base[digit], and then lane d moves base[d] past the trip.  Tiles, trips and waves are taken in row
//               order, equal digits keep their order: every pass is stable, hence the sort.
//   gather    dests[i][r] = sources[i][idx[r]] for every column of the sort in one launch, cut into tiles of 256 rows of ONE column as
//             wc_tiles does (wit_count.hip): the column index is workgroup-uniform and comes from the uploaded table through the scalar
//             cache.  A dest is never a source (create refuses it), so no word a launch writes is read by it.
//   memory    a scatter store and a gather load are guarded by `< rows`: whatever the table holds, nothing is accessed outside the
//             pair buffers and rows [0, rows) of the named columns.
// A one-sweep pass with decoupled look-back is not here: it would put a cross-workgroup spin into a new kernel for a gain nobody has
// measured (DESIGN §13 notes it as the follow-up).
// No inline assembly, nothing per lane in an array indexed at run time.
#include <algorithm>
#include <vector>

#include "wit_program_dev.hpp"

namespace bx {

constexpr uint32_t WS_LANES = 256, WS_WAVES = WS_LANES / 64, WS_TRIPS = 4, WS_TILE = WS_LANES * WS_TRIPS;
constexpr uint32_t WS_CHUNK = 8 * WS_LANES;  // table words per workgroup of the scan

// the key of one sort, by value: indexed by unrolled loops only
struct WsKeys {
    uint32_t n_keys, col[BX_WIT_MAX_SORT_KEYS], bits[BX_WIT_MAX_SORT_KEYS];
};
// the geometry of one pass: n_tiles tiles of WS_TILE rows, tiles_per_wg per workgroup; the digit is bits [shift, shift + 8) of the key
struct WsRun {
    uint32_t rows, shift, n_tiles, tiles_per_wg;
};

__global__ __launch_bounds__(WS_LANES) void wit_sort_pack_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ idx, const uint32_t* __restrict__ data, WsKeys k,
                                                                 uint32_t po2, uint32_t rows) {
    const uint32_t r = blockIdx.x * WS_LANES + threadIdx.x;
    if (r >= rows) return;
    uint64_t key = 0;
#pragma unroll
    for (uint32_t q = 0; q < BX_WIT_MAX_SORT_KEYS; ++q)
        if (q < k.n_keys) {  // bits in [1, 31]
            const uint32_t v = fp_decode(data[((size_t)k.col[q] << po2) + r]) & ((1u << k.bits[q]) - 1u);
            key = key << k.bits[q] | v;
        }
    keys[r] = key;
    idx[r] = r;
}

// the lanes of this wave that hold an element (`live`) with this lane's digit; called by whole waves.  A lane that is not live gets a
// mask it must not use.
__device__ __forceinline__ uint64_t ws_match(uint32_t digit, bool live) {
    uint64_t peers = __ballot(live);
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

__global__ __launch_bounds__(WS_LANES) void wit_sort_hist_kernel(uint32_t* __restrict__ table, const uint64_t* __restrict__ keys, WsRun g) {
    __shared__ uint32_t bins[256];
    const uint32_t t0 = blockIdx.x * g.tiles_per_wg;
    const uint32_t t1 = g.n_tiles - t0 < g.tiles_per_wg ? g.n_tiles : t0 + g.tiles_per_wg;  // the launch has t0 < n_tiles
    const uint64_t below = ((uint64_t)1 << __lane_id()) - 1;
    for (uint32_t t = t0; t < t1; ++t) {
        bins[threadIdx.x] = 0u;  // lane d owns bin d between the barriers
        __syncthreads();
#pragma unroll
        for (uint32_t trip = 0; trip < WS_TRIPS; ++trip) {
            const uint32_t r = t * WS_TILE + trip * WS_LANES + threadIdx.x;
            const bool live = r < g.rows;
            uint32_t digit = 0u;
            if (live) digit = (uint32_t)(keys[r] >> g.shift) & 0xFFu;
            const uint64_t peers = ws_match(digit, live);
            if (live && !(peers & below)) atomicAdd(&bins[digit], (uint32_t)__popcll(peers));
        }
        __syncthreads();
        table[(size_t)threadIdx.x * g.n_tiles + t] = bins[threadIdx.x];
    }
}

// exclusive scan of one value per lane over the workgroup's 256 lanes, `total` = the sum of all of them; wsum: WS_WAVES words of LDS
__device__ __forceinline__ uint32_t ws_wg_exscan(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < WS_WAVES; ++w) {
        const uint32_t s = wsum[w];
        if (w < wave) before += s;
        total += s;
    }
    __syncthreads();  // wsum may be written again
    return before + inc - v;
}

// m, the table's length, is a multiple of 256: a lane's eight words are all below m or all at or above it
__global__ __launch_bounds__(WS_LANES) void wit_sort_sums_kernel(uint32_t* __restrict__ sums, const uint32_t* __restrict__ table, uint32_t m) {
    __shared__ uint32_t wsum[WS_WAVES];
    const uint32_t i = blockIdx.x * WS_CHUNK + threadIdx.x * 8u;
    uint32_t s = 0u;
    if (i < m) {
        const uint4 a = *(const uint4*)(table + i), b = *(const uint4*)(table + i + 4);
        s = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
    }
    uint32_t total;
    (void)ws_wg_exscan(s, wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(WS_LANES) void wit_sort_scan_kernel(uint32_t* __restrict__ table, const uint32_t* __restrict__ sums, uint32_t m) {
    __shared__ uint32_t wsum[WS_WAVES];
    uint32_t part = 0u, offset, total;
    for (uint32_t j = threadIdx.x; j < blockIdx.x; j += WS_LANES) part += sums[j];  // the chunks before this one
    (void)ws_wg_exscan(part, wsum, offset);
    const uint32_t i = blockIdx.x * WS_CHUNK + threadIdx.x * 8u;
    const bool in = i < m;
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (in) a = *(const uint4*)(table + i), b = *(const uint4*)(table + i + 4);
    uint32_t x = offset + ws_wg_exscan(a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w, wsum, total);
    if (!in) return;
    uint4 oa, ob;
    oa.x = x, x += a.x;
    oa.y = x, x += a.y;
    oa.z = x, x += a.z;
    oa.w = x, x += a.w;
    ob.x = x, x += b.x;
    ob.y = x, x += b.y;
    ob.z = x, x += b.z;
    ob.w = x;
    *(uint4*)(table + i) = oa;
    *(uint4*)(table + i + 4) = ob;
}

__global__ __launch_bounds__(WS_LANES) void wit_sort_scatter_kernel(uint64_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out, const uint64_t* __restrict__ keys_in,
                                                                    const uint32_t* __restrict__ idx_in, const uint32_t* __restrict__ table, WsRun g) {
    __shared__ uint32_t base[256];             // where the next element of each digit goes
    __shared__ uint32_t wcnt[WS_WAVES * 256];  // per wave: its elements of each digit in the current trip
    const uint32_t t0 = blockIdx.x * g.tiles_per_wg;
    const uint32_t t1 = g.n_tiles - t0 < g.tiles_per_wg ? g.n_tiles : t0 + g.tiles_per_wg;
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t below = ((uint64_t)1 << __lane_id()) - 1;
#pragma unroll
    for (uint32_t w = 0; w < WS_WAVES; ++w) wcnt[w * 256u + threadIdx.x] = 0u;
    for (uint32_t t = t0; t < t1; ++t) {
        base[threadIdx.x] = table[(size_t)threadIdx.x * g.n_tiles + t];  // lane d owns base[d] and wcnt[.][d] outside the middle phase
        __syncthreads();
        for (uint32_t trip = 0; trip < WS_TRIPS; ++trip) {
            const uint32_t r = t * WS_TILE + trip * WS_LANES + threadIdx.x;
            const bool live = r < g.rows;
            uint64_t key = 0u;
            uint32_t id = 0u;
            if (live) key = keys_in[r], id = idx_in[r];
            const uint32_t digit = (uint32_t)(key >> g.shift) & 0xFFu;
            const uint64_t peers = ws_match(digit, live);
            const uint32_t rank = (uint32_t)__popcll(peers & below);
            if (live && rank == 0u) wcnt[wave * 256u + digit] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (live) {
                uint32_t dst = base[digit] + rank;
#pragma unroll
                for (uint32_t w = 0; w + 1 < WS_WAVES; ++w)
                    if (w < wave) dst += wcnt[w * 256u + digit];
                if (dst < g.rows) keys_out[dst] = key, idx_out[dst] = id;
            }
            __syncthreads();
            uint32_t s = 0u;
#pragma unroll
            for (uint32_t w = 0; w < WS_WAVES; ++w) {
                s += wcnt[w * 256u + threadIdx.x];
                wcnt[w * 256u + threadIdx.x] = 0u;
            }
            base[threadIdx.x] += s;
            __syncthreads();
        }
    }
}

// cols = [sources (n_cols) | dests (n_cols)]; workgroup = one tile of 256 rows of one column
__global__ __launch_bounds__(WS_LANES) void wit_sort_gather_kernel(uint32_t* data, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ cols, uint32_t n_cols,
                                                                   uint32_t tiles_per_col, uint32_t po2, uint32_t rows) {
    const uint32_t q = blockIdx.x / tiles_per_col, r = (blockIdx.x - q * tiles_per_col) * WS_LANES + threadIdx.x;
    if (r >= rows) return;
    const uint32_t* src = data + ((size_t)cols[q] << po2);
    uint32_t* dst = data + ((size_t)cols[n_cols + q] << po2);
    const uint32_t j = idx[r];
    if (j < rows) dst[r] = src[j];
}

const char* wit_sorts_load(bx_ctx* c, bx_wit_program_dev* d, const bx_wit_program* prog) {
    d->sorts = prog->sorts;
    if (d->sorts.empty()) return nullptr;
    for (const WitSort& s : d->sorts) {
        d->sort_col_off.push_back(d->sort_flat.size());
        d->sort_flat.insert(d->sort_flat.end(), s.sources.begin(), s.sources.end());
        d->sort_flat.insert(d->sort_flat.end(), s.dests.begin(), s.dests.end());
    }
    BX_TRY(d->sort_cols.alloc(c, d->sort_flat.size()));
    // the caller waits for the stream before sort_flat can go away (it lives as long as the loaded program anyway)
    BX_HIP(c, hipMemcpyAsync(d->sort_cols.b.dptr, d->sort_flat.data(), d->sort_flat.size() * 4, hipMemcpyHostToDevice, c->stream));
    return nullptr;
}

namespace {
uint32_t ws_tiles(size_t rows) { return (uint32_t)((rows + WS_TILE - 1) / WS_TILE); }
uint32_t ws_chunks(uint32_t n_tiles) { return (256u * n_tiles + WS_CHUNK - 1) / WS_CHUNK; }  // 256 * n_tiles <= 2^22
}  // namespace

const char* wit_sorts_run(bx_ctx* c, bx_wit_program_dev* d, uint32_t po2, bx_buf data) {
    if (d->sorts.empty()) return nullptr;
    const uint32_t n = 1u << po2;
    size_t need = 0;  // the caller has checked every sort against N and w_data
    for (const WitSort& s : d->sorts) need = std::max<size_t>(need, s.rows ? s.rows : n);
    if (need > d->sort_cap) {  // the work space of the largest sort: two buffers of `need` keys and indices, the digit table and its chunk sums
        BX_HIP(c, stream_wait(c));  // an earlier run may still use the smaller one
        DevBuf pairs, table;
        BX_TRY(pairs.alloc(c, 6 * need));
        BX_TRY(table.alloc(c, (size_t)256 * ws_tiles(need) + ws_chunks(ws_tiles(need))));
        d->sort_pairs = std::move(pairs);
        d->sort_table = std::move(table);
        d->sort_cap = need;
    }
    const size_t cap = d->sort_cap;
    uint64_t* const keys[2] = {(uint64_t*)d->sort_pairs.b.dptr, (uint64_t*)d->sort_pairs.b.dptr + cap};  // 8-byte aligned: the keys come first
    uint32_t* const idx[2] = {(uint32_t*)d->sort_pairs.b.dptr + 4 * cap, (uint32_t*)d->sort_pairs.b.dptr + 5 * cap};
    uint32_t* const dtab = (uint32_t*)d->sort_table.b.dptr;
    for (size_t k = 0; k < d->sorts.size(); ++k) {
        const WitSort& s = d->sorts[k];
        const uint32_t rows = s.rows ? s.rows : n, n_cols = (uint32_t)s.sources.size();
        WsKeys wk{};
        wk.n_keys = (uint32_t)s.bits.size();
        uint32_t total_bits = 0;
        for (uint32_t q = 0; q < wk.n_keys; ++q) wk.col[q] = s.sources[q], wk.bits[q] = s.bits[q], total_bits += s.bits[q];
        const uint32_t passes = (total_bits + 7) / 8, row_wgs = (rows + WS_LANES - 1) / WS_LANES;
        {
            OpScope op(c, "wit_program_sort_pack", (double)rows * (4.0 * wk.n_keys + 12.0));
            hipLaunchKernelGGL(wit_sort_pack_kernel, dim3(row_wgs), dim3(WS_LANES), 0, c->stream, keys[0], idx[0], (const uint32_t*)data.dptr, wk, po2, rows);
            BX_LAUNCH_CHECK(c);
        }
        {
            WsRun g;
            g.rows = rows, g.n_tiles = ws_tiles(rows);
            // at least two tiles per workgroup when there are that many, at most four workgroups per CU
            uint32_t wgs = std::min((g.n_tiles + 1) / 2, 4u * (uint32_t)c->cu_count);
            g.tiles_per_wg = (g.n_tiles + wgs - 1) / wgs;
            wgs = (g.n_tiles + g.tiles_per_wg - 1) / g.tiles_per_wg;  // no workgroup without a tile
            const uint32_t m = 256u * g.n_tiles, chunks = ws_chunks(g.n_tiles);
            uint32_t* const sums = dtab + m;
            // per pass: the keys twice and the indices once in, both out, the table written, scanned and read
            OpScope op(c, "wit_program_sort", (double)passes * (32.0 * rows + 16.0 * m));
            for (uint32_t p = 0; p < passes; ++p) {
                g.shift = 8 * p;
                const uint32_t in = p & 1u, out = in ^ 1u;
                hipLaunchKernelGGL(wit_sort_hist_kernel, dim3(wgs), dim3(WS_LANES), 0, c->stream, dtab, (const uint64_t*)keys[in], g);
                BX_LAUNCH_CHECK(c);
                hipLaunchKernelGGL(wit_sort_sums_kernel, dim3(chunks), dim3(WS_LANES), 0, c->stream, sums, (const uint32_t*)dtab, m);
                BX_LAUNCH_CHECK(c);
                hipLaunchKernelGGL(wit_sort_scan_kernel, dim3(chunks), dim3(WS_LANES), 0, c->stream, dtab, (const uint32_t*)sums, m);
                BX_LAUNCH_CHECK(c);
                hipLaunchKernelGGL(wit_sort_scatter_kernel, dim3(wgs), dim3(WS_LANES), 0, c->stream, keys[out], idx[out], (const uint64_t*)keys[in],
                                   (const uint32_t*)idx[in], (const uint32_t*)dtab, g);
                BX_LAUNCH_CHECK(c);
            }
        }
        const uint32_t tiles_per_col = row_wgs;
        OpScope op(c, "wit_program_sort_gather", (double)rows * (4.0 + 8.0 * n_cols));
        hipLaunchKernelGGL(wit_sort_gather_kernel, dim3(n_cols * tiles_per_col), dim3(WS_LANES), 0, c->stream, (uint32_t*)data.dptr, (const uint32_t*)idx[passes & 1u],
                           (const uint32_t*)d->sort_cols.b.dptr + d->sort_col_off[k], n_cols, tiles_per_col, po2, rows);
        BX_LAUNCH_CHECK(c);
    }
    return nullptr;
}

}  // namespace bx
