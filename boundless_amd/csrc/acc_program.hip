// acc_program.hip — device half of accumulate programs ("Accumulate programs" of include/bx_program.h is the normative text;
// cons_program.hpp the compiled form): a kernel that gathers the columns a program taps before the prover interpolates them away, and a
// kernel that INTERPRETS the program's instruction stream over the N trace rows and writes every sequence's per-row term where the
// HAL's scans take it (bx_logup_accumulate, bx_batch_prefix_products, bx_batch_ratio_products).  The interpreter follows the choices of cons_program.hip, for
// the reasons written at the top of that file, and shares its opcode bodies (cons_program_exec.hpp):
//   lanes     one lane per row, 256 per workgroup; lanes past N return at once
//   slots     narrow and wide slot files in dynamic LDS, slot-major, sized per program (narrow + 4 wide KiB, at most 128 KiB)
//   barriers  none: a lane only ever touches its own column of the slot files, and `kept` is read-only here
//   state     nothing per lane is held in an array indexed at run time: a value is in LDS or in flight
//   stream    wave-uniform, through a const __restrict__ pointer, CP_FETCH instructions per fetch, decoded through readfirstlane
//   values    canonical throughout, the same fp_* / f4_* calls: bx_acc_program_run_host gives identical words
//   memory    a tap is kept[k N + ((r - back) & (N - 1))].  A term is ONE 16-byte store at run_ext[4 (s N + r)] — a base value is
//             promoted to (v, 0, 0, 0) — so a wave writes 1 KiB contiguous; a sum also writes one word at mults[s N + r]; the t-th
//             ratio's denominator is the term of sequence S + t, behind the S sequences the store reads
#define BX_PLAIN_MAD 1
#include <memory>
#include <new>
#include <vector>

#include "acc_program_dev.hpp"
#include "circuit_common.hpp"
#include "cons_program_exec.hpp"

namespace bx {

// kept column k = column kept_cols[k].y of group kept_cols[k].x, whole
__global__ void acc_program_keep_kernel(uint32_t* __restrict__ kept, const uint32_t* __restrict__ code, const uint32_t* __restrict__ data,
                                        const uint2* __restrict__ kept_cols, uint32_t po2, uint32_t n_kept) {
    const uint32_t n = 1u << po2;
    const size_t total = (size_t)n_kept << po2, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint2 kc = kept_cols[i >> po2];
        kept[i] = (kc.x == 0 ? code : data)[((size_t)kc.y << po2) + (i & (n - 1))];
    }
}

// what cp_exec asks of this kernel: a tap is a kept column at row r - back; the opcodes cp_exec does not know are the term stores
struct AccEnv {
    static constexpr bool MIX = false, EXT = true;
    const uint32_t* __restrict__ kept;
    const uint2* __restrict__ taps;  // (kept index, back)
    uint32_t* __restrict__ run_ext;
    uint32_t* __restrict__ mults;
    uint32_t n, r;
    __device__ __forceinline__ uint32_t tap(uint32_t imm) const {
        const uint2 t = taps[imm];
        return kept[(size_t)t.x * n + ((r - t.y) & (n - 1u))];  // N divides 2^32: the wrapped difference reduces properly
    }
    __device__ __forceinline__ const uint32_t* mixpows() const { return nullptr; }
    __device__ __forceinline__ void term(uint32_t s, const Fp4& v) const {
        *reinterpret_cast<uint4*>(run_ext + 4 * ((size_t)s * n + r)) = make_uint4(v.c[0], v.c[1], v.c[2], v.c[3]);
    }
    __device__ __forceinline__ void other(uint32_t op, uint32_t a, uint32_t b, uint32_t imm, uint32_t* nar, uint32_t* wid) const {
        switch (op) {
        case CP_TSUM_B:
            term(imm, Fp4{{nar[b * CP_LANES], 0u, 0u, 0u}});
            mults[(size_t)imm * n + r] = nar[a * CP_LANES];
            break;
        case CP_TSUM_E:
            term(imm, cp_ldw(wid, b));
            mults[(size_t)imm * n + r] = nar[a * CP_LANES];
            break;
        case CP_TPROD_B: term(imm, Fp4{{nar[a * CP_LANES], 0u, 0u, 0u}}); break;
        case CP_TPROD_E: term(imm, cp_ldw(wid, a)); break;
        case CP_TDEN_B: term(imm, Fp4{{nar[a * CP_LANES], 0u, 0u, 0u}}); break;  // a ratio's denominator: sequences [S, S + R) of run_ext
        case CP_TDEN_E: term(imm, cp_ldw(wid, a)); break;
        default: break;
        }
    }
};

__global__ __launch_bounds__(256) void acc_program_kernel(uint32_t* __restrict__ run_ext, uint32_t* __restrict__ mults, const uint32_t* __restrict__ kept,
                                                          const uint4* __restrict__ code, const uint2* __restrict__ taps, const uint32_t* __restrict__ scal,
                                                          uint32_t n, uint32_t n_fetch, uint32_t n_narrow) {
    extern __shared__ uint32_t slots[];
    const uint32_t r = blockIdx.x * CP_LANES + threadIdx.x;
    if (r >= n) return;
    uint32_t* const nar = slots + threadIdx.x;                        // narrow slot s: nar[256 s]
    uint32_t* const wid = slots + n_narrow * CP_LANES + threadIdx.x;  // wide slot s, plane k: wid[256 (4 s + k)]
    const AccEnv env{kept, taps, run_ext, mults, n, r};

    static_assert(CP_FETCH == 4, "the fetch below reads two uint4 = four instructions");
    for (uint32_t f = 0; f < n_fetch; ++f) {
        const uint4 lo = code[2 * (size_t)f], hi = code[2 * (size_t)f + 1];
        cp_exec(lo.x, lo.y, nar, wid, scal, env);
        cp_exec(lo.z, lo.w, nar, wid, scal, env);
        cp_exec(hi.x, hi.y, nar, wid, scal, env);
        cp_exec(hi.z, hi.w, nar, wid, scal, env);
    }
}

namespace {
LoadedPrograms<bx_acc_program_dev> g_loaded;  // what bx_free still has to release
}  // namespace

void acc_programs_release(bx_ctx* c) {
    for (bx_acc_program_dev* d : g_loaded.take_all(c)) delete d;  // the caller has drained the stream
}
}  // namespace bx

extern "C" const char* bx_acc_program_load(bx_ctx* c, const bx_acc_program* prog, bx_acc_program_dev** out) try {
    using namespace bx;
    if (!c) return "bx_acc_program_load: null ctx";
    BX_REQUIRE(c, prog && out, "bx_acc_program_load: null argument");
    BX_ENTER(c);
    *out = nullptr;
    // the compiler refuses what does not fit; a stream from anywhere else must not reach the kernel
    BX_REQUIRE(c, program_fits(prog), "bx_acc_program_load: the program's stream or counts are outside the device limits");
    std::unique_ptr<bx_acc_program_dev> d(new bx_acc_program_dev());
    d->ctx = c;
    d->info = prog->info;
    d->ratios = prog->ratios;
    d->n_fetch = (uint32_t)(prog->code.size() / (2 * CP_FETCH));
    d->kept_cols = prog->kept;
    d->lds = (size_t)(prog->info.narrow + 4 * prog->info.wide) * CP_LANES * 4;
    BX_TRY(upload_program(
        c, d->code, d->taps, d->scal, prog->code, prog->taps,
        [&](uint32_t* w, size_t t, const bx_cons_tap& tp) { w[0] = prog->tap_kept[t], w[1] = tp.back; }, prog->consts, prog->info.n_globals + 4));
    // the kept table, after everything above is allocated and has landed: no copy is ever in flight when an allocation fails
    BX_TRY(d->kept.alloc(c, prog->kept.empty() ? 2 : 2 * prog->kept.size()));
    std::vector<uint32_t> keptw(2 * prog->kept.size());
    for (size_t k = 0; k < prog->kept.size(); ++k) {
        keptw[2 * k] = prog->kept[k].group;
        keptw[2 * k + 1] = prog->kept[k].col;
    }
    if (!keptw.empty()) {
        BX_HIP(c, hipMemcpyAsync(d->kept.b.dptr, keptw.data(), keptw.size() * 4, hipMemcpyHostToDevice, c->stream));
        BX_HIP(c, stream_wait(c));  // keptw goes away
    }
    BX_REQUIRE(c, reserve_slot_lds((const void*)acc_program_kernel, d->lds), "bx_acc_program_load: the slot files' LDS could not be reserved");
    g_loaded.insert(c, d.get());
    *out = d.release();
    return nullptr;
} BX_ABI_CATCH(c, "bx_acc_program_load")

extern "C" const char* bx_acc_program_unload(bx_acc_program_dev* dev) try {
    using namespace bx;
    if (!dev) return nullptr;
    bx_ctx* c = g_loaded.take(dev);
    if (!c) return "bx_acc_program_unload: not a loaded program (unloaded twice, or its ctx was freed)";
    (void)hipSetDevice(c->device);
    (void)stream_wait(c);  // a launch may still read the tables
    delete dev;
    return nullptr;
} BX_ABI_CATCH(nullptr, "bx_acc_program_unload")

extern "C" const char* bx_acc_program_keep(bx_ctx* c, bx_acc_program_dev* dev, uint32_t po2, bx_buf code, uint32_t w_code, bx_buf data, uint32_t w_data,
                                           bx_buf kept) try {
    using namespace bx;
    if (!c) return "bx_acc_program_keep: null ctx";
    BX_REQUIRE(c, dev != nullptr, "bx_acc_program_keep: null argument");
    BX_REQUIRE(c, dev->ctx == c, "bx_acc_program_keep: the program was loaded on another ctx");
    BX_REQUIRE(c, po2 >= 1 && po2 <= 24, "bx_acc_program_keep: po2 must be in [1, 24]");
    BX_ENTER(c);
    const size_t n = (size_t)1 << po2, K = dev->info.kept;
    BX_REQUIRE(c, code.len == n * w_code && data.len == n * w_data && kept.len == n * K,
               "bx_acc_program_keep: buffer size mismatch (groups N x width, kept N x the program's kept columns)");
    if (const char* e = acc_program_check_widths(dev->kept_cols, "bx_acc_program_keep", w_code, w_data)) return set_msg(c, e);
    BX_REQUIRE(c, !bufs_overlap(kept, code), "bx_acc_program_keep: kept and code overlap");
    BX_REQUIRE(c, !bufs_overlap(kept, data), "bx_acc_program_keep: kept and data overlap");
    if (!K) return nullptr;
    OpScope op(c, "acc_program_keep", 8.0 * (double)(n * K));
    hipLaunchKernelGGL(acc_program_keep_kernel, dim3(grid_for(n * K)), dim3(256), 0, c->stream, (uint32_t*)kept.dptr, (const uint32_t*)code.dptr,
                       (const uint32_t*)data.dptr, (const uint2*)dev->kept.b.dptr, po2, (uint32_t)K);
    BX_LAUNCH_CHECK(c);
    return nullptr;
} BX_ABI_CATCH(c, "bx_acc_program_keep")

extern "C" const char* bx_acc_program_run(bx_ctx* c, bx_acc_program_dev* dev, uint32_t po2, bx_buf kept, const uint32_t* globals, const uint32_t mix[4],
                                          bx_buf run_ext, bx_buf mults, bx_buf accum, uint32_t w_accum) try {
    using namespace bx;
    if (!c) return "bx_acc_program_run: null ctx";
    BX_REQUIRE(c, dev && mix, "bx_acc_program_run: null argument");
    BX_REQUIRE(c, dev->ctx == c, "bx_acc_program_run: the program was loaded on another ctx");
    BX_REQUIRE(c, po2 >= 1 && po2 <= 24, "bx_acc_program_run: po2 must be in [1, 24]");
    BX_ENTER(c);
    const size_t n = (size_t)1 << po2, K = dev->info.kept, S = dev->info.sequences, sums = dev->info.sums, R = dev->ratios;
    const uint32_t ng = dev->info.n_globals;
    BX_REQUIRE(c, !ng || globals, "bx_acc_program_run: the program names globals and none were given");
    BX_REQUIRE(c, kept.len == n * K, "bx_acc_program_run: kept size mismatch (N x the program's kept columns)");
    BX_REQUIRE(c, R || run_ext.len == 4 * n * S, "bx_acc_program_run: run_ext size mismatch (4 N words per sequence)");
    BX_REQUIRE(c, run_ext.len == 4 * n * (S + R), "bx_acc_program_run: run_ext size mismatch (4 N words per sequence and 4 N more per RATIO: its denominators)");
    BX_REQUIRE(c, mults.len == n * sums, "bx_acc_program_run: mults size mismatch (N words per running sum)");
    BX_REQUIRE(c, accum.len == n * w_accum, "bx_acc_program_run: accum size mismatch (N x w_accum)");
    if (w_accum < 4 * S) {
        snprintf(c->err, sizeof c->err, "bx_acc_program_run: the program writes %zu accum columns, the accum group has %u", 4 * S, w_accum);
        return c->err;
    }
    BX_REQUIRE(c, ((uintptr_t)run_ext.dptr & 15u) == 0, "bx_acc_program_run: run_ext must be 16-byte aligned");
    BX_REQUIRE(c, !bufs_overlap(run_ext, mults), "bx_acc_program_run: run_ext and mults overlap");
    BX_REQUIRE(c, !bufs_overlap(run_ext, accum), "bx_acc_program_run: run_ext and accum overlap");
    BX_REQUIRE(c, !bufs_overlap(run_ext, kept), "bx_acc_program_run: run_ext and kept overlap");
    BX_REQUIRE(c, !bufs_overlap(mults, accum), "bx_acc_program_run: mults and accum overlap");
    BX_REQUIRE(c, !bufs_overlap(mults, kept), "bx_acc_program_run: mults and kept overlap");
    BX_REQUIRE(c, !bufs_overlap(accum, kept), "bx_acc_program_run: accum and kept overlap");
    uint32_t dyn[BX_MAX_GLOBALS + 4];
    for (uint32_t k = 0; k < ng; ++k) dyn[k] = globals[k];
    for (uint32_t k = 0; k < 4; ++k) dyn[ng + k] = mix[k];
    BX_TRY(h2d_staged(c, dev->scal.slice(0, ng + 4), dyn, ng + 4));
    {
        // every tap is read once; a term is 16 bytes, and 4 more for a sum
        OpScope op(c, "acc_program_run", 4.0 * (double)n * ((double)dev->info.taps + 4.0 * (double)(S + R) + (double)sums));
        hipLaunchKernelGGL(acc_program_kernel, dim3((unsigned)((n + CP_LANES - 1) / CP_LANES)), dim3(CP_LANES), dev->lds, c->stream, (uint32_t*)run_ext.dptr,
                           (uint32_t*)mults.dptr, (const uint32_t*)kept.dptr, (const uint4*)dev->code.b.dptr, (const uint2*)dev->taps.b.dptr,
                           (const uint32_t*)dev->scal.b.dptr, (uint32_t)n, dev->n_fetch, dev->info.narrow);
        BX_LAUNCH_CHECK(c);
    }
    uint32_t* const run = (uint32_t*)run_ext.dptr;
    if (sums) {  // in place: the sums replace the denominators
        const bx_buf part{run, 4 * n * sums};
        BX_TRY(bx_logup_accumulate(c, part, part, mults, sums));
    }
    if (S - R > sums) BX_TRY(bx_batch_prefix_products(c, bx_buf{run + 4 * n * sums, 4 * n * (S - R - sums)}, S - R - sums));
    if (R) {  // in place: the products replace the numerators; the denominators lie right behind them
        const bx_buf nums{run + 4 * n * (S - R), 4 * n * R};
        BX_TRY(bx_batch_ratio_products(c, nums, nums, bx_buf{run + 4 * n * S, 4 * n * R}, R));
    }
    OpScope op(c, "acc_program_store", 32.0 * (double)(n * S));
    return store_ext_columns(c, accum, run_ext, po2, (uint32_t)S, (uint32_t)(4 * S), 0);  // no filler: columns >= 4 S are not written
} BX_ABI_CATCH(c, "bx_acc_program_run")
