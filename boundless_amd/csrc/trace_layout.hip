// trace_layout.hip — device half of trace layouts (include/bx_layout.h, "Trace layouts", is the normative text; trace_layout.hpp holds
// what a code cell is and the per-column table): a layout loaded on a ctx, the two kernels, and the device entries of the base table.
//   layout_code_kernel   the code group, column-major, cut into tiles of 256 rows of ONE column as wc_tiles does (wit_count.hip): the
//                        column's kind and operands are workgroup-uniform and come from the uploaded table through the scalar cache
//   layout_place_kernel  the free cells: row-major records -> column-major Montgomery words.  A workgroup of 256 lanes takes 64
//                        consecutive records.  Their 64 * stride words are contiguous in the payload and are read coalesced, one dword
//                        per lane (the payload begins at word 7 of the segment: 4-byte aligned only), into LDS at an ODD row pitch
//                        (stride | 1): the 64 lanes of a wave that read one word of 64 consecutive records then hit 32 distinct banks
//                        per half-wave.  After one barrier each wave walks every fourth column of the per-column table (wave-uniform,
//                        scalar loads): lane = row; read the word, shift, mask, one fp_mul by R^2, and one 256-byte store per wave.
//                        Rows in [R, A) take the encoded pad, rows >= A the noise word; a column without a field is an entry of the
//                        same table (mask 0, pad 0), not a second launch; a tile wholly at or above R loads nothing.
//   memory               a load of the payload is guarded by the tile's record count, a store by r < N and c < w_data; the entry
//                        points check the payload's length against the segment buffer and the groups against N x width first.
// At the largest stride the tile is 64 x 129 words = 33 024 bytes of LDS: below what a kernel may use by default.
// No inline assembly, nothing per lane in an array indexed at run time.
#define BX_PLAIN_MAD 1
#include <memory>
#include <new>
#include <vector>

#include "circuit_common.hpp"
#include "program_loaded.hpp"
#include "trace_layout.hpp"

namespace bx {

constexpr uint32_t LC_ROWS = 256;  // rows of a code tile = lanes of its workgroup
constexpr uint32_t LP_ROWS = 64;   // records of a place tile: lane = row within a wave
constexpr uint32_t LP_LANES = 256;

__global__ __launch_bounds__(LC_ROWS) void layout_code_kernel(uint32_t* __restrict__ code, const bx_layout_code_col* __restrict__ cols,
                                                              const uint32_t* __restrict__ table, uint32_t n, uint32_t act, uint32_t tiles_per_col) {
    const uint32_t c = blockIdx.x / tiles_per_col, t = blockIdx.x - c * tiles_per_col;  // workgroup-uniform; the launch has c < n_code
    const uint32_t r = t * LC_ROWS + threadIdx.x;
    if (r >= n) return;
    const bx_layout_code_col k = cols[c];
    code[(size_t)c * n + r] = layout_code_cell(k, table, c, r, n, act);
}

struct PlaceRun {
    uint32_t w_data, stride, pitch;  // pitch = stride | 1: words between two records in LDS
    uint32_t n, act, records;        // N, A, R
    uint64_t nseed;                  // nseed_1
};

__global__ __launch_bounds__(LP_LANES) void layout_place_kernel(uint32_t* __restrict__ data, const uint32_t* __restrict__ payload,
                                                                const uint4* __restrict__ columns, PlaceRun g) {
    const uint32_t r0 = blockIdx.x * LP_ROWS;
#if defined(BX_LAYOUT_PLACE_STRIDED)
    // The comparison build of tools/layout_bench.py, never the library's: no tile, every lane reads its own record's words from memory
    // (64 lanes, 64 addresses `stride` words apart).  profiles/r30_trace_layout.json holds both figures.
    const uint32_t* mine = payload + (size_t)(r0 + (threadIdx.x & 63u)) * g.stride;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#else
    extern __shared__ uint32_t lp_tile[];  // LP_ROWS records of g.pitch words
    const uint32_t have = g.records > r0 ? (g.records - r0 < LP_ROWS ? g.records - r0 : LP_ROWS) : 0u;  // this tile's records: workgroup-uniform
    if (have) {
        const uint32_t* src = payload + (size_t)r0 * g.stride;
        const uint32_t words = have * g.stride;
        for (uint32_t i = threadIdx.x; i < words; i += LP_LANES) {
            const uint32_t row = i / g.stride;
            lp_tile[row * g.pitch + (i - row * g.stride)] = src[i];
        }
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t* mine = lp_tile + lane * g.pitch;
#endif
    const uint32_t r = r0 + lane;
    if (r >= g.n) return;
    for (uint32_t c = wave; c < g.w_data; c += LP_LANES / 64) {
        const uint4 k = columns[c];  // word, shift, mask, pad
        uint32_t cell;
        if (r >= g.act) cell = synth_word(g.nseed, c, r);
        else if (r < g.records) cell = fp_mul(R2, (mine[k.x] >> k.y) & k.z);  // a value below 2^30 < P
        else cell = k.w;
        data[(size_t)c * g.n + r] = cell;
    }
}

}  // namespace bx

// a layout loaded on a ctx
struct bx_trace_layout_dev {
    bx_ctx* ctx = nullptr;
    std::unique_ptr<bx_trace_layout> layout;  // a copy of what the kernels and the shape checks need: the caller's layout may go first
    bx::DevBuf code_cols, table;              // 3 words per code column; the PERIODIC values
    bx::DevBuf columns;                       // the per-column table of the last place, 4 words per data column; grown on demand
    uint32_t columns_wd = UINT32_MAX;         // the w_data it was built for
};

namespace bx {
namespace {
LoadedPrograms<bx_trace_layout_dev> g_loaded;  // what bx_free still has to release
}  // namespace

void trace_layouts_release(bx_ctx* c) {
    for (bx_trace_layout_dev* d : g_loaded.take_all(c)) delete d;  // the caller has drained the stream
}
}  // namespace bx

extern "C" const char* bx_trace_layout_load(bx_ctx* c, const bx_trace_layout* layout, bx_trace_layout_dev** out) try {
    using namespace bx;
    if (!c) return "bx_trace_layout_load: null ctx";
    BX_REQUIRE(c, layout && out, "bx_trace_layout_load: null argument");
    BX_ENTER(c);
    *out = nullptr;
    std::unique_ptr<bx_trace_layout_dev> d(new bx_trace_layout_dev());
    d->ctx = c;
    d->layout.reset(new bx_trace_layout());
    bx_trace_layout& l = *d->layout;
    l.code = layout->code, l.table = layout->table, l.fields = layout->fields;
    l.stride = layout->stride, l.noise_rows = layout->noise_rows, l.n_globals = layout->n_globals, l.min_w_data = layout->min_w_data;
    static_assert(sizeof(bx_layout_code_col) == 12, "a code column is three words on the device");
    BX_TRY(d->code_cols.alloc(c, 3 * l.code.size()));
    BX_TRY(d->table.alloc(c, std::max<size_t>(l.table.size(), 1)));
    BX_HIP(c, hipMemcpyAsync(d->code_cols.b.dptr, l.code.data(), 12 * l.code.size(), hipMemcpyHostToDevice, c->stream));
    if (!l.table.empty()) BX_HIP(c, hipMemcpyAsync(d->table.b.dptr, l.table.data(), 4 * l.table.size(), hipMemcpyHostToDevice, c->stream));
    BX_HIP(c, stream_wait(c));  // the copies read the dev's own vectors: pageable memory
    g_loaded.insert(c, d.get());
    *out = d.release();
    return nullptr;
} BX_ABI_CATCH(c, "bx_trace_layout_load")

extern "C" const char* bx_trace_layout_unload(bx_trace_layout_dev* dev) try {
    using namespace bx;
    if (!dev) return nullptr;
    bx_ctx* c = g_loaded.take(dev);
    if (!c) return "bx_trace_layout_unload: not a loaded layout (unloaded twice, or its ctx was freed)";
    (void)hipSetDevice(c->device);
    (void)stream_wait(c);  // a launch may still read the tables
    delete dev;
    return nullptr;
} BX_ABI_CATCH(nullptr, "bx_trace_layout_unload")

extern "C" const char* bx_trace_layout_code(bx_ctx* c, bx_trace_layout_dev* dev, uint32_t po2, bx_buf code) try {
    using namespace bx;
    if (!c) return "bx_trace_layout_code: null ctx";
    BX_REQUIRE(c, dev != nullptr, "bx_trace_layout_code: null argument");
    BX_REQUIRE(c, dev->ctx == c, "bx_trace_layout_code: the layout was loaded on another ctx");
    BX_REQUIRE(c, po2 >= 1 && po2 <= 24, "bx_trace_layout_code: po2 must be in [1, 24]");
    BX_ENTER(c);
    const bx_trace_layout& l = *dev->layout;
    const size_t n = (size_t)1 << po2;
    BX_REQUIRE(c, code.len == n * l.code.size(), "bx_trace_layout_code: buffer size mismatch (code N x n_code)");
    if (const char* e = layout_check_shape(&l, po2, "bx_trace_layout_code", c->err, sizeof c->err)) return e;
    const size_t tiles_per_col = (n + LC_ROWS - 1) / LC_ROWS, tiles = tiles_per_col * l.code.size();
    BX_REQUIRE(c, tiles <= 0x7FFFFFFFu, "bx_trace_layout_code: the code group is too large for one launch");
    OpScope op(c, "layout_code", 4.0 * (double)code.len);
    hipLaunchKernelGGL(layout_code_kernel, dim3((unsigned)tiles), dim3(LC_ROWS), 0, c->stream, (uint32_t*)code.dptr, (const bx_layout_code_col*)dev->code_cols.b.dptr,
                       (const uint32_t*)dev->table.b.dptr, (uint32_t)n, layout_active_rows(po2, l.noise_rows), (uint32_t)tiles_per_col);
    BX_LAUNCH_CHECK(c);
    return nullptr;
} BX_ABI_CATCH(c, "bx_trace_layout_code")

extern "C" const char* bx_trace_layout_place(bx_ctx* c, bx_trace_layout_dev* dev, uint32_t po2, bx_buf segment_dev, size_t segment_len, uint64_t noise_seed,
                                             bx_buf data, uint32_t w_data) try {
    using namespace bx;
    const char* who = "bx_trace_layout_place";
    if (!c) return "bx_trace_layout_place: null ctx";
    BX_REQUIRE(c, dev != nullptr, "bx_trace_layout_place: null argument");
    BX_REQUIRE(c, dev->ctx == c, "bx_trace_layout_place: the layout was loaded on another ctx");
    BX_REQUIRE(c, po2 >= 1 && po2 <= 24, "bx_trace_layout_place: po2 must be in [1, 24]");
    BX_ENTER(c);
    const bx_trace_layout& l = *dev->layout;
    const size_t n = (size_t)1 << po2;
    BX_REQUIRE(c, w_data <= 65535 && data.len == n * w_data, "bx_trace_layout_place: buffer size mismatch (data N x w_data, at most 65535 columns)");
    if (w_data < l.min_w_data) {
        snprintf(c->err, sizeof c->err, "%s: w_data is %u, a field names data column %u", who, w_data, l.min_w_data - 1);
        return c->err;
    }
    uint32_t records = 0;
    if (const char* e = layout_check_payload(&l, po2, segment_len, who, &records, c->err, sizeof c->err)) return e;
    BX_REQUIRE(c, segment_dev.len >= (segment_len + 3) / 4, "bx_trace_layout_place: buffer size mismatch (segment_dev holds fewer words than segment_len bytes)");
    BX_REQUIRE(c, !bufs_overlap(segment_dev, data), "bx_trace_layout_place: segment_dev and data overlap");
    if (!w_data) return nullptr;
    if (dev->columns_wd != w_data) {  // the per-column table of this width, through the pinned ring: no wait
        if (dev->columns.b.len < 4 * (size_t)w_data) {
            DevBuf grown;
            BX_TRY(grown.alloc(c, 4 * (size_t)w_data));
            dev->columns = std::move(grown);  // hipFree of the old table waits for the launches that read it
        }
        dev->columns_wd = UINT32_MAX;
        const std::vector<LayoutColumn> cols = l.columns(w_data);
        static_assert(sizeof(LayoutColumn) == 16, "a column entry is one uint4 on the device");
        BX_TRY(h2d_staged(c, dev->columns.slice(0, 4 * (size_t)w_data), (const uint32_t*)cols.data(), 4 * (size_t)w_data));
        dev->columns_wd = w_data;
    }
    PlaceRun g;
    g.w_data = w_data, g.stride = l.stride, g.pitch = l.stride | 1u;
    g.n = (uint32_t)n, g.act = layout_active_rows(po2, l.noise_rows), g.records = records;
    g.nseed = data_seed(noise_seed);
    // the payload is read once, every data cell written once
    OpScope op(c, "layout_place", 4.0 * ((double)records * l.stride + (double)data.len));
    hipLaunchKernelGGL(layout_place_kernel, dim3((unsigned)((n + LP_ROWS - 1) / LP_ROWS)), dim3(LP_LANES), (size_t)LP_ROWS * g.pitch * 4, c->stream, (uint32_t*)data.dptr,
                       (const uint32_t*)segment_dev.dptr + BX_SEGMENT_WIRE_BYTES / 4, (const uint4*)dev->columns.b.dptr, g);
    BX_LAUNCH_CHECK(c);
    return nullptr;
} BX_ABI_CATCH(c, "bx_trace_layout_place")

// ---------------------------------------------------------------------------------------------------------------------
// the device entries of a layout's base table (the host entries: trace_layout_host.cpp)
// ---------------------------------------------------------------------------------------------------------------------
namespace bx {
namespace {
struct LayoutState {
    bx_trace_layout_dev* dev = nullptr;
    bx_segment_params shape{};
    uint64_t seed = 0;
    NoiseSeed noise;
};
void lt_destroy(void*, void* state) {
    LayoutState* st = (LayoutState*)state;
    if (!st) return;
    (void)bx_trace_layout_unload(st->dev);
    delete st;
}
const char* lt_create(void* user, bx_ctx* c, const bx_segment_params* shape, void** state) {
    bx_trace_layout* l = (bx_trace_layout*)user;
    bx_segment_params checked = *shape;  // the prover normalised it already; a direct caller of the table may not have
    if (const char* e = l->ops.normalize(l, &checked)) return set_msg(c, e);
    std::unique_ptr<LayoutState> st(new (std::nothrow) LayoutState());
    BX_REQUIRE(c, st != nullptr, "trace layout: out of host memory");
    st->shape = *shape;
    BX_TRY(bx_trace_layout_load(c, l, &st->dev));
    *state = st.release();
    return nullptr;
}
const char* lt_code_group(void*, void* state, bx_ctx* c, bx_buf code) {
    LayoutState* st = (LayoutState*)state;
    return bx_trace_layout_code(c, st->dev, st->shape.po2, code);
}
void lt_set_noise_seed(void*, void* state, uint64_t noise_seed) { ((LayoutState*)state)->noise.set(noise_seed); }
const char* lt_witgen(void* user, void* state, bx_ctx* c, bx_buf /*code*/, bx_buf data, const uint8_t* segment, size_t segment_len, bx_buf segment_dev,
                      uint32_t* globals_out) {
    LayoutState* st = (LayoutState*)state;
    uint64_t seed = 0;
    const char* refused = segment_header(c, segment, segment_len, st->shape.po2, &seed);
    const uint64_t noise = st->noise.take(seed);  // a noise seed given through set_noise_seed belongs to THIS witgen, accepted or refused
    if (refused) return refused;
    BX_TRY(bx_trace_layout_place(c, st->dev, st->shape.po2, segment_dev, segment_len, noise, data, st->shape.w_data));
    st->seed = seed;
    for (uint32_t k = 0; k < ((bx_trace_layout*)user)->n_globals; ++k) globals_out[k] = 0u;
    return nullptr;
}
const char* lt_accumulate(void*, void* state, bx_ctx* c, bx_buf accum, const uint32_t mix[4]) {
    LayoutState* st = (LayoutState*)state;
    const size_t n = (size_t)1 << st->shape.po2;
    BX_REQUIRE(c, accum.len == n * st->shape.w_accum, "trace layout: accumulate: accum group buffer size mismatch");
    OpScope op(c, "layout_filler", 4.0 * (double)accum.len);
    return store_ext_columns(c, accum, bx_buf{nullptr, 0}, st->shape.po2, 0, st->shape.w_accum, filler_seed(st->seed, mix));  // no ext runs: filler alone
}
void lt_device_entries(bx_circuit_ops* ops) {
    ops->create = lt_create;
    ops->destroy = lt_destroy;
    ops->code_group = lt_code_group;
    ops->witgen = lt_witgen;
    ops->accumulate = lt_accumulate;
    ops->set_noise_seed = lt_set_noise_seed;
}
// what bx_trace_layout_create (trace_layout_host.cpp) calls for every layout of a library that has this translation unit
[[maybe_unused]] bool lt_registered = (g_layout_device_entries = lt_device_entries, true);
}  // namespace
}  // namespace bx
