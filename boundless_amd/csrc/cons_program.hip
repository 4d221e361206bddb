// cons_program.hip — device half of constraint programs (include/bx_program.h is the normative text; cons_program.hpp the compiled
// form): a kernel that INTERPRETS a program's instruction stream over the 4N domain, and the bx_circuit_ops table made of a program
// and a base table (whose witgen may be completed by a witness program, wit_program.hip, and whose accumulate by an accumulate program,
// acc_program.hip).  One instruction's opcode bodies are in cons_program_exec.hpp, shared with acc_program.hip.
//   lanes     one lane per domain point, 256 per workgroup
//   slots     the two slot files live in LDS, slot-major: narrow slot s is words [256 s, 256 s + 256) (1 KiB), wide slot s four such
//             planes (4 KiB).  A wave's access to a slot is 64 consecutive dwords: conflict-free.  A lane only ever touches its own
//             column, so there is NO barrier, and lanes past the domain return at once.  The dynamic LDS is sized per program
//             (narrow + 4 wide KiB; at most 32 + 96 = 128 KiB of the CU's 160), so a small program keeps several workgroups per CU.
//   state     nothing per lane is held in an array indexed at run time (that would be scratch): a value is in LDS or in flight
//   stream    wave-uniform: fetched through a const __restrict__ pointer indexed by the loop counter, CP_FETCH instructions per
//             fetch, so that it comes through the scalar cache; decode and dispatch are scalar (readfirstlane makes it explicit)
//   values    canonical throughout: fp_add / fp_sub / fp_mul, f4_scale and f4_mul_lz (canonical in, canonical out — its lazy
//             accumulators do not outlive one product, lazy_ext.hpp).  Nothing lazy is kept across instructions, so there is no bound
//             to carry.  Mix powers come from the canonical half of mix_power_table.
#define BX_PLAIN_MAD 1
#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "circuit_common.hpp"
#include "cons_program.hpp"
#include "acc_program_dev.hpp"
#include "cons_program_dev.hpp"
#include "cons_program_exec.hpp"

namespace bx {

struct ConsLaunch {
    uint32_t zinv[4];  // 1 / (3^N w_4^m - 1), m = row mod 4
    uint32_t dom, n_fetch, n_narrow, ret_slot;
};

// what cp_exec (cons_program_exec.hpp) asks of this kernel: a tap is a column of the 4N evaluations at row i - 4 back
struct ConsEnv {
    static constexpr bool MIX = true, EXT = true;
    const uint32_t* __restrict__ ecode;
    const uint32_t* __restrict__ edata;
    const uint32_t* __restrict__ eacc;
    const uint2* __restrict__ taps;
    const uint32_t* __restrict__ pows;
    uint32_t dom, i;
    __device__ __forceinline__ uint32_t tap(uint32_t imm) const {
        const uint2 t = taps[imm];
        const uint32_t g = t.y >> 30, back = t.y & 0x3FFFFFFFu;
        const uint32_t* __restrict__ col = (g == 0 ? ecode : (g == 1 ? edata : eacc)) + (size_t)t.x * dom;
        return col[(i - 4u * back) & (dom - 1u)];  // dom divides 2^32: the wrapped difference reduces properly
    }
    __device__ __forceinline__ const uint32_t* mixpows() const { return pows; }
    __device__ __forceinline__ void other(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*, uint32_t*) const {}
};

__global__ __launch_bounds__(256) void cons_program_kernel(uint32_t* __restrict__ check, const uint32_t* __restrict__ ecode,
                                                           const uint32_t* __restrict__ edata, const uint32_t* __restrict__ eacc,
                                                           const uint4* __restrict__ code, const uint2* __restrict__ taps,
                                                           const uint32_t* __restrict__ scal, const uint32_t* __restrict__ mixpows, ConsLaunch L) {
    extern __shared__ uint32_t slots[];
    const uint32_t dom = L.dom;
    const uint32_t i = blockIdx.x * CP_LANES + threadIdx.x;
    if (i >= dom) return;
    uint32_t* const nar = slots + threadIdx.x;                          // narrow slot s: nar[256 s]
    uint32_t* const wid = slots + L.n_narrow * CP_LANES + threadIdx.x;  // wide slot s, plane k: wid[256 (4 s + k)]

    const ConsEnv env{ecode, edata, eacc, taps, mixpows, dom, i};

    static_assert(CP_FETCH == 4, "the fetch below reads two uint4 = four instructions");
    for (uint32_t f = 0; f < L.n_fetch; ++f) {
        const uint4 lo = code[2 * (size_t)f], hi = code[2 * (size_t)f + 1];
        cp_exec(lo.x, lo.y, nar, wid, scal, env);
        cp_exec(lo.z, lo.w, nar, wid, scal, env);
        cp_exec(hi.x, hi.y, nar, wid, scal, env);
        cp_exec(hi.z, hi.w, nar, wid, scal, env);
    }
    const Fp4 q = f4_scale(cp_ldw(wid, L.ret_slot), L.zinv[i & 3u]);
#pragma unroll
    for (int k = 0; k < 4; ++k) check[(size_t)k * dom + i] = q.c[k];
}

}  // namespace bx

// a program loaded on a ctx: bx_cons_program_dev (cons_program_dev.hpp)

namespace bx {
namespace {
LoadedPrograms<bx_cons_program_dev> g_loaded;  // what bx_free still has to release
}  // namespace

void cons_programs_release(bx_ctx* c) {
    for (bx_cons_program_dev* d : g_loaded.take_all(c)) {  // the caller has drained the stream
        gen_release(d->gen);
        delete d;
    }
}
}  // namespace bx

extern "C" const char* bx_cons_program_load(bx_ctx* c, const bx_cons_program* prog, bx_cons_program_dev** out) try {
    using namespace bx;
    if (!c) return "bx_cons_program_load: null ctx";
    BX_REQUIRE(c, prog && out, "bx_cons_program_load: null argument");
    BX_ENTER(c);
    *out = nullptr;
    // the compiler refuses what does not fit; a stream from anywhere else must not reach the kernel
    BX_REQUIRE(c, program_fits(prog), "bx_cons_program_load: the program's slot counts are outside the device limits");
    std::unique_ptr<bx_cons_program_dev> d(new bx_cons_program_dev());
    d->ctx = c;
    d->info = prog->info;
    d->n_pows = prog->n_pows;
    d->ret_slot = prog->ret_slot;
    d->n_fetch = (uint32_t)(prog->code.size() / (2 * CP_FETCH));
    for (int g = 0; g < 3; ++g) d->max_col[g] = prog->max_col[g];
    BX_TRY(bx_cons_program_digest(prog, d->gen.digest));  // what a generated kernel must have been built from (attach_kernel)
    d->lds = (size_t)(prog->info.narrow + 4 * prog->info.wide) * CP_LANES * 4;
    BX_TRY(d->mixpows.alloc(c, 8 * (size_t)prog->n_pows));
    BX_TRY(upload_program(
        c, d->code, d->taps, d->scal, prog->code, prog->taps,
        [](uint32_t* w, size_t, const bx_cons_tap& t) { w[0] = t.col, w[1] = t.back | t.group << 30; }, prog->consts, prog->info.n_globals + 4));
    BX_REQUIRE(c, reserve_slot_lds((const void*)cons_program_kernel, d->lds), "bx_cons_program_load: the slot files' LDS could not be reserved");
    g_loaded.insert(c, d.get());
    *out = d.release();
    return nullptr;
} BX_ABI_CATCH(c, "bx_cons_program_load")

extern "C" const char* bx_cons_program_unload(bx_cons_program_dev* dev) try {
    using namespace bx;
    if (!dev) return nullptr;
    bx_ctx* c = g_loaded.take(dev);
    if (!c) return "bx_cons_program_unload: not a loaded program (unloaded twice, or its ctx was freed)";
    (void)hipSetDevice(c->device);
    (void)stream_wait(c);  // a launch may still read the tables
    gen_release(dev->gen);
    delete dev;
    return nullptr;
} BX_ABI_CATCH(nullptr, "bx_cons_program_unload")

extern "C" const char* bx_cons_program_eval_check(bx_ctx* c, bx_cons_program_dev* dev, uint32_t po2, bx_buf check, bx_buf code_eval, uint32_t w_code,
                                                  bx_buf data_eval, uint32_t w_data, bx_buf accum_eval, uint32_t w_accum, const uint32_t poly_mix[4],
                                                  const uint32_t mix[4], const uint32_t* globals, uint32_t n_globals) try {
    using namespace bx;
    if (!c) return "bx_cons_program_eval_check: null ctx";
    BX_REQUIRE(c, dev && poly_mix && mix, "bx_cons_program_eval_check: null argument");
    BX_REQUIRE(c, dev->ctx == c, "bx_cons_program_eval_check: the program was loaded on another ctx");
    BX_REQUIRE(c, po2 >= 1 && po2 <= 24, "bx_cons_program_eval_check: po2 must be in [1, 24]");
    BX_ENTER(c);
    const size_t dom = (size_t)4 << po2;
    BX_REQUIRE(c, check.len == 4 * dom && code_eval.len == dom * w_code && data_eval.len == dom * w_data && accum_eval.len == dom * w_accum,
               "bx_cons_program_eval_check: buffer size mismatch (check 16N, groups 4N x width)");
    const uint32_t widths[3] = {w_code, w_data, w_accum};
    for (int g = 0; g < 3; ++g)
        if (dev->max_col[g] > widths[g]) {
            snprintf(c->err, sizeof c->err, "bx_cons_program_eval_check: the program taps column %u of group %d, which has %u columns", dev->max_col[g] - 1, g, widths[g]);
            return c->err;
        }
    const uint32_t ng = dev->info.n_globals;
    if (n_globals < ng || (ng && !globals)) {
        snprintf(c->err, sizeof c->err, "bx_cons_program_eval_check: %u globals given, the program needs %u", globals ? n_globals : 0u, ng);
        return c->err;
    }
    uint32_t dyn[BX_MAX_GLOBALS + 4];
    for (uint32_t k = 0; k < ng; ++k) dyn[k] = globals[k];
    for (uint32_t k = 0; k < 4; ++k) dyn[ng + k] = mix[k];
    BX_TRY(h2d_staged(c, dev->scal.slice(0, ng + 4), dyn, ng + 4));
    BX_TRY(mix_power_table(c, dev->mixpows.b, poly_mix, dev->n_pows));
    ConsLaunch L;
    vanishing_inverses(po2, L.zinv);
    if (dev->gen.fn) return cons_gen_launch(c, dev, po2, L.zinv, check, code_eval, data_eval, accum_eval);  // the generated kernel, when one is attached
    L.dom = (uint32_t)dom;
    L.n_fetch = dev->n_fetch;
    L.n_narrow = dev->info.narrow;
    L.ret_slot = dev->ret_slot;
    // every tap is read once, four planes are written
    OpScope op(c, "cons_program_eval_check", 4.0 * (double)dom * ((double)dev->info.taps + 4.0));
    hipLaunchKernelGGL(cons_program_kernel, dim3((unsigned)((dom + CP_LANES - 1) / CP_LANES)), dim3(CP_LANES), dev->lds, c->stream, (uint32_t*)check.dptr,
                       (const uint32_t*)code_eval.dptr, (const uint32_t*)data_eval.dptr, (const uint32_t*)accum_eval.dptr, (const uint4*)dev->code.b.dptr,
                       (const uint2*)dev->taps.b.dptr, (const uint32_t*)dev->scal.b.dptr, (const uint32_t*)dev->mixpows.b.dptr, L);
    BX_LAUNCH_CHECK(c);
    return nullptr;
} BX_ABI_CATCH(c, "bx_cons_program_eval_check")

// ---------------------------------------------------------------------------------------------------------------------
// a bx_circuit_ops made of a program (taps, eval_check, constraints_at) and a base table (everything else)
// ---------------------------------------------------------------------------------------------------------------------
struct bx_cons_circuit {
    bx_circuit_ops ops{};
    const bx_circuit_ops* base = nullptr;
    const bx_cons_program* prog = nullptr;
    std::vector<uint8_t> kernel;  // bx_cons_circuit_set_kernel: the code object create attaches (empty = the interpreter)
    const bx_wit_program* wit = nullptr;  // bx_cons_circuit_set_witness: witgen derives columns and global cells from it (NULL = base alone)
    std::vector<uint8_t> wit_kernel;  // bx_cons_circuit_set_witness_kernel: the code object create attaches to `wit` (empty = the interpreter)
    const bx_acc_program* acc = nullptr;  // bx_cons_circuit_set_accumulate: accumulate's columns [0, 4 S) come from it (NULL = base alone)
};

namespace bx {
namespace {
struct ConsState {
    void* base_state = nullptr;
    bx_cons_program_dev* dev = nullptr;
    bx_wit_program_dev* wit_dev = nullptr;
    bx_acc_program_dev* acc_dev = nullptr;
    bx_segment_params shape{};
    uint32_t n_globals = 0;
    // the accumulate program's: the tapped columns as witgen left them, the scans' work space, and witgen's public words
    DevBuf kept, run_ext, mults;
    uint32_t globals[BX_MAX_GLOBALS] = {};
};
const char* cc_normalize(void* u, bx_segment_params* shape) {
    const bx_circuit_ops* b = ((bx_cons_circuit*)u)->base;
    return b->normalize ? b->normalize(b->user, shape) : nullptr;
}
uint32_t cc_taps(void* u, const bx_segment_params*, int group, uint32_t col, uint32_t* backs_out) {
    return bx_cons_program_taps(((bx_cons_circuit*)u)->prog, group, col, backs_out);
}
uint32_t cc_n_globals(void* u, const bx_segment_params* shape) {
    const bx_circuit_ops* b = ((bx_cons_circuit*)u)->base;
    return b->n_globals ? b->n_globals(b->user, shape) : 0;
}
void cc_destroy(void* u, void* state) {
    const bx_circuit_ops* b = ((bx_cons_circuit*)u)->base;
    ConsState* st = (ConsState*)state;
    if (!st) return;
    (void)bx_cons_program_unload(st->dev);
    (void)bx_wit_program_unload(st->wit_dev);
    (void)bx_acc_program_unload(st->acc_dev);
    if (st->base_state && b->destroy) b->destroy(b->user, st->base_state);
    delete st;
}
const char* cc_create(void* u, bx_ctx* c, const bx_segment_params* shape, void** state) {
    bx_cons_circuit* cc = (bx_cons_circuit*)u;
    const bx_circuit_ops* b = cc->base;
    const uint32_t widths[3] = {shape->w_code, shape->w_data, shape->w_accum};
    for (int g = 0; g < 3; ++g)
        if (cc->prog->max_col[g] > widths[g]) {
            snprintf(c->err, sizeof c->err, "cons circuit: the program taps column %u of group %d, the shape has %u columns there", cc->prog->max_col[g] - 1, g, widths[g]);
            return c->err;
        }
    const uint32_t ng = cc_n_globals(u, shape);
    if (ng != cc->prog->info.n_globals) {
        snprintf(c->err, sizeof c->err, "cons circuit: the program has %u globals, the base circuit %u", cc->prog->info.n_globals, ng);
        return c->err;
    }
    BX_REQUIRE(c, cc->wit || cc->wit_kernel.empty(), "cons circuit: a witness kernel is set but no witness program (bx_cons_circuit_set_witness)");
    if (const bx_wit_program* w = cc->wit) {  // the witness program against the shape, before anything is loaded
        if (const char* e = wit_program_check_widths(w->max_col, w->max_set, "cons circuit: witness program", shape->w_code, shape->w_data)) return set_msg(c, e);
        if (const char* e = wit_program_check_sorts(w->sorts, "cons circuit: witness program", shape->po2, shape->w_data)) return set_msg(c, e);
        if (const char* e = wit_program_check_counts(w->counts, "cons circuit: witness program", shape->po2, shape->w_data)) return set_msg(c, e);
        for (size_t k = 0; k < w->cells.size(); ++k) {
            const bx_wit_global_cell& g = w->cells[k];
            if (g.col >= shape->w_data)
                snprintf(c->err, sizeof c->err, "cons circuit: witness program: global cell %zu reads data column %u, the shape has %u columns there", k, g.col, shape->w_data);
            else if (g.row >> shape->po2)
                snprintf(c->err, sizeof c->err, "cons circuit: witness program: global cell %zu reads row %u, the trace has %u rows", k, g.row, 1u << shape->po2);
            else if (g.global >= ng)
                snprintf(c->err, sizeof c->err, "cons circuit: witness program: global cell %zu names global %u, the base circuit has %u", k, g.global, ng);
            else
                continue;
            return c->err;
        }
    }
    if (const bx_acc_program* a = cc->acc) {  // the accumulate program against the shape, before anything is loaded
        if (const char* e = acc_program_check_widths(a->kept, "cons circuit: accumulate program", shape->w_code, shape->w_data)) return set_msg(c, e);
        const uint32_t cols = 4 * a->info.sequences;
        if (cols > shape->w_accum) {
            snprintf(c->err, sizeof c->err, "cons circuit: accumulate program: %u sequences need %u accum columns, the shape has %u", a->info.sequences, cols,
                     shape->w_accum);
            return c->err;
        }
        if (a->info.n_globals != ng) {
            snprintf(c->err, sizeof c->err, "cons circuit: accumulate program: the program has %u globals, the base circuit %u", a->info.n_globals, ng);
            return c->err;
        }
        if (!b->accumulate && shape->w_accum > cols) {
            snprintf(c->err, sizeof c->err, "cons circuit: accumulate program: accum columns %u .. %u are not the program's and the base circuit has no accumulate", cols,
                     shape->w_accum - 1);
            return c->err;
        }
    }
    std::unique_ptr<ConsState> st(new (std::nothrow) ConsState());
    BX_REQUIRE(c, st != nullptr, "cons circuit: out of host memory");
    st->shape = *shape;
    st->n_globals = ng;
    BX_TRY(bx_cons_program_load(c, cc->prog, &st->dev));
    const auto undo = [&](const char* e) {  // keeps the message, unloads what this create loaded
        const char* kept = e == c->err ? e : set_msg(c, e);
        (void)bx_cons_program_unload(st->dev);
        (void)bx_wit_program_unload(st->wit_dev);
        (void)bx_acc_program_unload(st->acc_dev);
        return kept;
    };
    if (!cc->kernel.empty())
        if (const char* e = bx_cons_program_attach_kernel(st->dev, cc->kernel.data(), cc->kernel.size())) return undo(e);
    if (cc->wit)
        if (const char* e = bx_wit_program_load(c, cc->wit, &st->wit_dev)) return undo(e);
    if (!cc->wit_kernel.empty())
        if (const char* e = bx_wit_program_attach_kernel(st->wit_dev, cc->wit_kernel.data(), cc->wit_kernel.size())) return undo(e);
    if (const bx_acc_program* a = cc->acc) {
        if (const char* e = bx_acc_program_load(c, a, &st->acc_dev)) return undo(e);
        const size_t n = (size_t)1 << shape->po2;
        for (const char* e : {st->kept.alloc(c, std::max<size_t>(n * a->info.kept, 1)), st->run_ext.alloc(c, 4 * n * (a->info.sequences + a->ratios)),  // a RATIO's denominators behind the S terms
                              st->mults.alloc(c, std::max<size_t>(n * a->info.sums, 1))})
            if (e) return undo(e);
    }
    if (b->create)
        if (const char* e = b->create(b->user, c, shape, &st->base_state)) return undo(e);
    *state = st.release();
    return nullptr;
}
const char* cc_code_group(void* u, void* state, bx_ctx* c, bx_buf code) {
    const bx_circuit_ops* b = ((bx_cons_circuit*)u)->base;
    BX_REQUIRE(c, b->code_group != nullptr, "cons circuit: the base circuit has no code_group");
    return b->code_group(b->user, ((ConsState*)state)->base_state, c, code);
}
const char* cc_witness(bx_cons_circuit* cc, const ConsState* st, bx_ctx* c, bx_buf code, bx_buf data, uint32_t* globals_out) {
    if (!st->wit_dev) return nullptr;
    // the base has placed the free cells: derive the rest, then take the public words that are cells of the trace
    BX_TRY(bx_wit_program_run(c, st->wit_dev, st->shape.po2, code, st->shape.w_code, data, st->shape.w_data));
    const std::vector<bx_wit_global_cell>& cells = cc->wit->cells;
    if (cells.empty()) return nullptr;
    const uint32_t* landed[BX_MAX_GLOBALS];
    size_t used = 0;
    for (size_t k = 0; k < cells.size(); ++k)  // create has checked column, row and index against the shape
        BX_TRY(d2h_batch_add(c, &used, bx_buf{(uint32_t*)data.dptr + ((size_t)cells[k].col << st->shape.po2) + cells[k].row, 1}, 1, &landed[k]));
    BX_TRY(d2h_batch_wait(c));
    for (size_t k = 0; k < cells.size(); ++k) globals_out[cells[k].global] = *landed[k];
    return nullptr;
}
const char* cc_witgen(void* u, void* state, bx_ctx* c, bx_buf code, bx_buf data, const uint8_t* segment, size_t segment_len, bx_buf segment_dev,
                      uint32_t* globals_out) {
    const bx_circuit_ops* b = ((bx_cons_circuit*)u)->base;
    BX_REQUIRE(c, b->witgen != nullptr, "cons circuit: the base circuit has no witgen");
    ConsState* st = (ConsState*)state;
    if (const char* e = b->witgen(b->user, st->base_state, c, code, data, segment, segment_len, segment_dev, globals_out)) return e;
    BX_TRY(cc_witness((bx_cons_circuit*)u, st, c, code, data, globals_out));
    if (!st->acc_dev) return nullptr;
    // the prover interpolates `code` and `data` in place after this: what accumulate's program taps is copied now, and the public
    // words are final
    for (uint32_t k = 0; k < st->n_globals; ++k) st->globals[k] = globals_out[k];
    return bx_acc_program_keep(c, st->acc_dev, st->shape.po2, code, st->shape.w_code, data, st->shape.w_data,
                               st->kept.slice(0, ((size_t)st->acc_dev->info.kept) << st->shape.po2));
}
const char* cc_accumulate(void* u, void* state, bx_ctx* c, bx_buf accum, const uint32_t mix[4]) {
    const bx_circuit_ops* b = ((bx_cons_circuit*)u)->base;
    ConsState* st = (ConsState*)state;
    if (!st->acc_dev) {
        BX_REQUIRE(c, b->accumulate != nullptr, "cons circuit: the base circuit has no accumulate");
        return b->accumulate(b->user, st->base_state, c, accum, mix);
    }
    // the base owns filler and every column at or above 4 S; whatever it leaves below is overwritten
    if (b->accumulate)
        if (const char* e = b->accumulate(b->user, st->base_state, c, accum, mix)) return e;
    const size_t n = (size_t)1 << st->shape.po2;
    const bx_acc_program_info& in = st->acc_dev->info;
    return bx_acc_program_run(c, st->acc_dev, st->shape.po2, st->kept.slice(0, n * in.kept), st->globals, mix, st->run_ext.b, st->mults.slice(0, n * in.sums), accum,
                              st->shape.w_accum);
}
const char* cc_eval_check(void*, void* state, bx_ctx* c, bx_buf check, bx_buf ecode, bx_buf edata, bx_buf eacc, const uint32_t poly_mix[4], const uint32_t mix[4],
                          const uint32_t* globals) {
    const ConsState* st = (const ConsState*)state;
    return bx_cons_program_eval_check(c, st->dev, st->shape.po2, check, ecode, st->shape.w_code, edata, st->shape.w_data, eacc, st->shape.w_accum, poly_mix, mix,
                                      globals, st->n_globals);
}
const char* cc_constraints_at(void* u, const bx_segment_params*, const bx_tap_reader* taps, const uint32_t poly_mix[4], const uint32_t mix[4],
                              const uint32_t* globals, uint32_t out[4]) {
    return bx_cons_program_constraints_at(((bx_cons_circuit*)u)->prog, taps, poly_mix, mix, globals, out);
}
void cc_set_noise_seed(void* u, void* state, uint64_t noise_seed) {
    const bx_circuit_ops* b = ((bx_cons_circuit*)u)->base;
    b->set_noise_seed(b->user, ((ConsState*)state)->base_state, noise_seed);
}
const char* cc_check_code(void* u, const bx_segment_params* shape, const uint32_t root[8]) {
    const bx_circuit_ops* b = ((bx_cons_circuit*)u)->base;
    return b->check_code(b->user, shape, root);
}
}  // namespace
}  // namespace bx

extern "C" const char* bx_cons_circuit_create(const bx_circuit_ops* base, const bx_cons_program* prog, bx_cons_circuit** out) try {
    if (!base || !prog || !out) return "bx_cons_circuit_create: null argument";
    bx_cons_circuit* cc = new bx_cons_circuit();
    cc->base = base;
    cc->prog = prog;
    // the optional members stay NULL when the base has none: a table without check_code verifies only against an explicit context
    cc->ops = bx_circuit_ops{cc,
                             "bx-cons-program",
                             bx::cc_normalize,
                             bx::cc_taps,
                             bx::cc_n_globals,
                             bx::cc_create,
                             bx::cc_destroy,
                             bx::cc_code_group,
                             bx::cc_witgen,
                             bx::cc_accumulate,
                             bx::cc_eval_check,
                             bx::cc_constraints_at,
                             base->set_noise_seed ? bx::cc_set_noise_seed : nullptr,
                             base->check_code ? bx::cc_check_code : nullptr};
    *out = cc;
    return nullptr;
} catch (...) {
    return "bx_cons_circuit_create: out of host memory";
}
extern "C" const char* bx_cons_circuit_set_kernel(bx_cons_circuit* cc, const void* image, size_t len) try {
    if (!cc || (len && !image)) return "bx_cons_circuit_set_kernel: null argument";
    cc->kernel.assign((const uint8_t*)image, (const uint8_t*)image + len);
    return nullptr;
} catch (...) {
    return "bx_cons_circuit_set_kernel: out of host memory";
}
extern "C" const char* bx_cons_circuit_set_witness(bx_cons_circuit* cc, const bx_wit_program* wit) {
    if (!cc) return "bx_cons_circuit_set_witness: null argument";
    cc->wit = wit;
    return nullptr;
}
extern "C" const char* bx_cons_circuit_set_accumulate(bx_cons_circuit* cc, const bx_acc_program* acc) {
    if (!cc) return "bx_cons_circuit_set_accumulate: null argument";
    cc->acc = acc;
    return nullptr;
}
extern "C" const char* bx_cons_circuit_set_witness_kernel(bx_cons_circuit* cc, const void* image, size_t len) try {
    if (!cc || (len && !image)) return "bx_cons_circuit_set_witness_kernel: null argument";
    cc->wit_kernel.assign((const uint8_t*)image, (const uint8_t*)image + len);
    return nullptr;
} catch (...) {
    return "bx_cons_circuit_set_witness_kernel: out of host memory";
}
extern "C" const bx_circuit_ops* bx_cons_circuit_ops(bx_cons_circuit* cc) { return cc ? &cc->ops : nullptr; }
extern "C" void bx_cons_circuit_destroy(bx_cons_circuit* cc) { delete cc; }
