// wit_program.hip — device half of witness programs ("Witness programs" of include/bx_program.h is the normative text; cons_program.hpp
// the compiled form): a kernel that INTERPRETS a program's instruction stream over the N trace rows and stores the derived data
// columns.  It follows the choices of the constraint interpreter (cons_program.hip), for the reasons written at the top of that file,
// and shares its opcode bodies (cons_program_exec.hpp).  What is its own:
//   lanes     one lane per row, 256 per workgroup; lanes past N return at once
//   slots     the narrow slot file alone, sized per program: at most 32 KiB of dynamic LDS, so several workgroups share a CU
//   barriers  none: a lane only ever touches its own column of the slot file, and no lane reads a word of `data` that this launch
//             writes (a derived cell is forwarded by the compiler, never loaded), so the result does not depend on scheduling
//   values    canonical throughout (fp_add / fp_sub / fp_mul): the host executor gives identical words
//   memory    a tap is col[(r - back) & (N - 1)]; a store is data[col * N + r]: one coalesced 256-byte line per wave
#define BX_PLAIN_MAD 1
#include <memory>
#include <new>
#include <vector>

#include "circuit_common.hpp"
#include "cons_program_exec.hpp"
#include "wit_program_dev.hpp"

namespace bx {

// what cp_exec asks of this kernel: a tap is a column of the trace at row r - back; the one opcode cp_exec does not know is the store.
// `data` is read (free columns) and written (derived ones) through the one pointer: never the same word, but the same buffer.
struct WitEnv {
    static constexpr bool MIX = false, EXT = false;
    const uint32_t* __restrict__ code;
    uint32_t* data;
    const uint2* __restrict__ taps;
    uint32_t n, r;
    __device__ __forceinline__ uint32_t tap(uint32_t imm) const {
        const uint2 t = taps[imm];
        const uint32_t back = t.y & 0x3FFFFFFFu;
        const uint32_t* col = ((t.y >> 30) == 0 ? code : data) + (size_t)t.x * n;
        return col[(r - back) & (n - 1u)];  // N divides 2^32: the wrapped difference reduces properly
    }
    __device__ __forceinline__ void other(uint32_t op, uint32_t a, uint32_t, uint32_t imm, uint32_t* nar, uint32_t*) const {
        if (op == CP_ST) data[(size_t)imm * n + r] = nar[a * CP_LANES];
    }
};

__global__ __launch_bounds__(256) void wit_program_kernel(uint32_t* data, const uint32_t* __restrict__ code, const uint4* __restrict__ stream,
                                                          const uint2* __restrict__ taps, const uint32_t* __restrict__ consts, uint32_t n, uint32_t n_fetch) {
    extern __shared__ uint32_t slots[];
    const uint32_t r = blockIdx.x * CP_LANES + threadIdx.x;
    if (r >= n) return;
    uint32_t* const nar = slots + threadIdx.x;  // slot s: nar[256 s]
    const WitEnv env{code, data, taps, n, r};

    static_assert(CP_FETCH == 4, "the fetch below reads two uint4 = four instructions");
    for (uint32_t f = 0; f < n_fetch; ++f) {
        const uint4 lo = stream[2 * (size_t)f], hi = stream[2 * (size_t)f + 1];
        cp_exec(lo.x, lo.y, nar, nullptr, consts, env);  // `scal` is the constants alone
        cp_exec(lo.z, lo.w, nar, nullptr, consts, env);
        cp_exec(hi.x, hi.y, nar, nullptr, consts, env);
        cp_exec(hi.z, hi.w, nar, nullptr, consts, env);
    }
}

}  // namespace bx

// a witness program loaded on a ctx: bx_wit_program_dev (wit_program_dev.hpp)

namespace bx {
namespace {
LoadedPrograms<bx_wit_program_dev> g_loaded;  // what bx_free still has to release
}  // namespace

void wit_programs_release(bx_ctx* c) {
    for (bx_wit_program_dev* d : g_loaded.take_all(c)) {  // the caller has drained the stream
        gen_release(d->gen);
        delete d;
    }
}
}  // namespace bx

extern "C" const char* bx_wit_program_load(bx_ctx* c, const bx_wit_program* prog, bx_wit_program_dev** out) try {
    using namespace bx;
    if (!c) return "bx_wit_program_load: null ctx";
    BX_REQUIRE(c, prog && out, "bx_wit_program_load: null argument");
    BX_ENTER(c);
    *out = nullptr;
    // the compiler refuses what does not fit; a stream from anywhere else must not reach the kernel
    BX_REQUIRE(c, program_fits(prog), "bx_wit_program_load: the program's slot count is outside the device limit");
    std::unique_ptr<bx_wit_program_dev> d(new bx_wit_program_dev());
    d->ctx = c;
    d->info = prog->info;
    d->n_fetch = (uint32_t)(prog->code.size() / (2 * CP_FETCH));
    for (int g = 0; g < 2; ++g) d->max_col[g] = prog->max_col[g];
    d->max_set = prog->max_set;
    BX_TRY(bx_wit_program_digest(prog, d->gen.digest));  // what a generated kernel must have been built from (attach_kernel)
    d->lds = (size_t)prog->info.narrow * CP_LANES * 4;  // at most 32 KiB: below what a kernel may use by default
    BX_TRY(upload_program(
        c, d->code, d->taps, d->consts, prog->code, prog->taps,
        [](uint32_t* w, size_t, const bx_cons_tap& t) { w[0] = t.col, w[1] = t.back | t.group << 30; }, prog->consts, 0));  // `scal` is the constants alone
    // the multiplicity columns' source table and counters (wit_count.hip), after everything above is allocated and has landed: its
    // one copy is the last thing it does, so no copy is ever in flight when an allocation fails
    BX_TRY(wit_counts_load(c, d.get(), prog));
    BX_HIP(c, stream_wait(c));
    BX_TRY(wit_sorts_load(c, d.get(), prog));  // the sorts' column table (wit_sort.hip), likewise: allocation, then its one copy
    BX_HIP(c, stream_wait(c));
    g_loaded.insert(c, d.get());
    *out = d.release();
    return nullptr;
} BX_ABI_CATCH(c, "bx_wit_program_load")

extern "C" const char* bx_wit_program_unload(bx_wit_program_dev* dev) try {
    using namespace bx;
    if (!dev) return nullptr;
    bx_ctx* c = g_loaded.take(dev);
    if (!c) return "bx_wit_program_unload: not a loaded program (unloaded twice, or its ctx was freed)";
    (void)hipSetDevice(c->device);
    (void)stream_wait(c);  // a launch may still read the tables
    gen_release(dev->gen);
    delete dev;
    return nullptr;
} BX_ABI_CATCH(nullptr, "bx_wit_program_unload")

extern "C" const char* bx_wit_program_run(bx_ctx* c, bx_wit_program_dev* dev, uint32_t po2, bx_buf code, uint32_t w_code, bx_buf data, uint32_t w_data) try {
    using namespace bx;
    if (!c) return "bx_wit_program_run: null ctx";
    BX_REQUIRE(c, dev != nullptr, "bx_wit_program_run: null argument");
    BX_REQUIRE(c, dev->ctx == c, "bx_wit_program_run: the program was loaded on another ctx");
    BX_REQUIRE(c, po2 >= 1 && po2 <= 24, "bx_wit_program_run: po2 must be in [1, 24]");
    BX_ENTER(c);
    const size_t n = (size_t)1 << po2;
    BX_REQUIRE(c, code.len == n * w_code && data.len == n * w_data, "bx_wit_program_run: buffer size mismatch (groups N x width)");
    if (const char* e = wit_program_check_widths(dev->max_col, dev->max_set, "bx_wit_program_run", w_code, w_data)) return set_msg(c, e);
    BX_REQUIRE(c, !bufs_overlap(code, data), "bx_wit_program_run: code and data overlap");
    if (const char* e = wit_program_check_sorts(dev->sorts, "bx_wit_program_run", po2, w_data)) return set_msg(c, e);
    if (const char* e = wit_program_check_counts(dev->counts, "bx_wit_program_run", po2, w_data)) return set_msg(c, e);
    if (dev->gen.fn) {  // the generated kernel, when one is attached
        BX_TRY(wit_gen_launch(c, dev, po2, code, data));
        BX_TRY(wit_sorts_run(c, dev, po2, data));
        return wit_counts_run(c, dev, po2, data);
    }
    {
        // every tap is read once, every derived column written once
        OpScope op(c, "wit_program_run", 4.0 * (double)n * ((double)dev->info.taps + (double)dev->info.sets));
        hipLaunchKernelGGL(wit_program_kernel, dim3((unsigned)((n + CP_LANES - 1) / CP_LANES)), dim3(CP_LANES), dev->lds, c->stream, (uint32_t*)data.dptr,
                           (const uint32_t*)code.dptr, (const uint4*)dev->code.b.dptr, (const uint2*)dev->taps.b.dptr, (const uint32_t*)dev->consts.b.dptr,
                           (uint32_t)n, dev->n_fetch);
        BX_LAUNCH_CHECK(c);
    }
    BX_TRY(wit_sorts_run(c, dev, po2, data));  // the sorted columns, after every row (wit_sort.hip)
    return wit_counts_run(c, dev, po2, data);  // the multiplicity columns, after the sorts (wit_count.hip)
} BX_ABI_CATCH(c, "bx_wit_program_run")
