// circuit.hip — device side of the synthetic circuit that stands in for risc0-circuit-rv32im under
// `ProverServer::prove_segment` (bento/crates/workflow/src/tasks/prove.rs:41-49): witness generation, the accumulate
// step and eval_check.  include/bx_prover.h ("The synthetic circuit") is the normative text; circuit.hpp holds the shape
// rules shared with the host verifier.  Upstream's counterparts are the machine-generated `witgen`/`step_exec`, `accum`
// and `eval_check` kernels of risc0-circuit-rv32im-sys 4.0.1 (reference Cargo.lock:8996), which are not vendored.
//
// All three stages are VALU-bound (no HBM or MFMA roofline applies): a derived cell / a constraint costs T*(G-2) reduced
// products and T multiply-adds for the terms, then one reduction and one multiply-add per group of terms that share their
// first factor (circuit_dev.hpp, the factored form: 16 groups at (48, 3)); for G <= 2, T*(G-1) products term by term.  At G = 4 the
// terms are instead products of two shared pair products (circuit_dev.hpp, the pair form): at T = 64, 44 reduced pair products and 64
// multiply-adds.  In every form the sum is one 64-bit chain that is folded (hi * R + lo, one multiply-add) where it would leave 64
// bits — 13 times at (64, 4) — and reduced once at the end (lazy_ext.hpp, fold_r).
// The loads around it are one coalesced dword per lane and column.
// The signed multiply-adds are left to the compiler in this translation unit (poseidon2.hip pins them as single asm
// statements because its loop-carried cells get widened): here the terms of a cell share their inner products (7 pool entries
// give at most 28 distinct pairs), and only un-pinned code lets hipcc find them, with none of the s_nops it places between
// adjacent asm statements.  Per cell, compiled, the factored form: 486 VALU instructions (368 multiply-class) at (T, G) = (64, 4)
// and 265 (127) at (48, 3); term by term they were 630 (474) and 389 (218).  The pair form takes (64, 4) down by another 75
// instructions per cell, 117 of them fewer multiply-class: witness_derive_kernel<64,4> 568 (368) -> 493 (251), eval_check_kernel<64,4>
// 1340 (657) -> 1265 (540).  Two things the un-pinned code must be kept from.  With a constant factor in sight hipcc turns a sum of
// r_i * R into (sum of r_i) * R, and two terms with a common factor into one product of a 64-bit sum, each with an emulated
// 64 x 32-bit product; and it reassociates a chain's sum so that the fold comes in through a 64-bit add.  So the fold multiplies by
// an opaque copy of R and every step of a chain hides its result from the optimiser (lazy_ext.hpp: fold_r, smad_chain, smad_r);
// and the walk keeps its pool centred in registers (DerivedRegs<true>) instead of centring all 16 entries per cell.  The walk's loop
// body per cell, VALU instructions (multiplies), with the levels as multiply-adds and the centred walk: witness_derive_kernel<64,4>
// 412 (251) -> 312 (274), eval_check_kernel<64,4> 467 (275) -> 367 (298); with the chain folded instead of reduced and rescaled:
// -> 262 (211) and 317 (235), 54 -> 46 and 78 -> 70 VGPRs (seven waves per SIMD in eval_check).  DESIGN.md §4 has the tables.
// eval_check's constraints behind the walk (the accumulators', the pairs', the two boundary ones) run on lazy_ext.hpp: the ext-valued
// ones are one weighted sum of unreduced values (WeightedExtAcc), the base-valued ones join the walk's in LazyExtAcc, itself one folded
// chain per component: per accumulator 321 -> 99 instructions, per pair 183 -> 54, the walk 317 -> 277 per cell, 70 -> 61 VGPRs (eight waves).
#define BX_PLAIN_MAD 1
#include <memory>
#include <new>

#include "circuit_common.hpp"
#include "circuit_dev.hpp"

namespace bx {

// ---- witness: code group (selectors + public control words) ----
// A function of the shape alone (SYNTH_CODE_SEED is a constant): its committed root is the circuit's control ID.
__global__ void witness_code_kernel(uint32_t* __restrict__ code, Circuit cc) {
    const uint32_t n = 1u << cc.po2;
    const size_t total = (size_t)n * cc.wc, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
        code[i] = synth_code_cell(cc, (uint32_t)(i >> cc.po2), (uint32_t)(i & (n - 1)));
}
// ---- witness: free data columns (the permuted copies 4p+3, p < pairs, are placed by Hal::scatter afterwards) ----
// Rows >= active_rows() are the ZK noise rows: drawn from the noise seed, in the permuted copies too.
__global__ void witness_free_kernel(uint32_t* __restrict__ data, Circuit cc, uint64_t gseed, uint64_t nseed) {
    const uint32_t n = 1u << cc.po2, act = cc.active_rows();
    const size_t total = (size_t)n * cc.F, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t c = (uint32_t)(i >> cc.po2), r = (uint32_t)(i & (n - 1));
        if (r < act && (c & 3u) == 3u && (c >> 2) < cc.pairs) continue;
        data[i] = synth_word(r < act ? gseed : nseed, c, r);
    }
}
// offsets of pair p's scatter: entry r of column 4p+2 goes to column 4p+3, row perm_p(r) — relative to that column, which is the
// scatter's `into` (the whole group buffer would contain `values`, column 4p+2: bx_hal.h, "Operand overlap")   (built once per prover)
__global__ void perm_offsets_kernel(uint32_t* __restrict__ offsets, uint32_t* __restrict__ index, Circuit cc) {
    const uint32_t n = 1u << cc.po2, act = cc.active_rows();
    const size_t total = (size_t)n * cc.pairs, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t p = (uint32_t)(i >> cc.po2), r = (uint32_t)(i & (n - 1));
        offsets[i] = r < act ? cc.perm_row(p, r) : 0u;
    }
    // one entry per active cycle, none for the noise cycles
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) index[i] = (uint32_t)(i < act ? i : act);
}

// ---- witness: derived data columns, one thread per row, columns in order (column F+j reads F+j-1 .. F+j-4) ----
template <int TT, int GG>
__global__ __launch_bounds__(256) void witness_derive_kernel(uint32_t* __restrict__ data, const uint32_t* __restrict__ code, Circuit cc) {
    const uint32_t n = 1u << cc.po2;
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t rb1 = (r + n - 1) & (n - 1), rb2 = (r + n - 2) & (n - 1);
    // the compiled constraint sums walk over centred registers (a word is centred where it enters them), <0, 0> over canonical ones
    using Regs = DerivedRegs<(TT > 0)>;
    using word = typename Regs::word;
    const auto code_at = [&](unsigned i) -> word {
        const int col = cc.csel_col(i);
        return Regs::enter(col < 0 ? MONT_ONE : code[(size_t)col * n + r]);
    };
    Regs w;
#pragma unroll
    for (int q = 0; q < 8; ++q) w.ring[q] = code_at((unsigned)q);
#pragma unroll
    for (int q = 0; q < 3; ++q) w.u[q] = Regs::enter(data[(size_t)((uint32_t)q % cc.F) * n + r]);
#pragma unroll
    for (int q = 0; q < 4; ++q) w.k[q] = code_at((unsigned)q);
    for (uint32_t j = 0; j < cc.J; ++j) {
        word pool[Circuit::POOL];
        const int sb = Circuit::slot1_back(j);
        w.fill(pool, sb == 0 ? w.u[0] : Regs::enter(data[(size_t)j * n + (sb == 1 ? rb1 : rb2)]));
        const uint32_t d = cons_sum<TT, GG>(pool, cc.T, cc.G);
        data[(size_t)(cc.F + j) * n + r] = d;  // canonical, as every word in memory
        w.shift(Regs::enter(d), Regs::enter(data[(size_t)((j + 3) % cc.F) * n + r]), code_at(j + 4));
    }
}

// ---- accumulate: the columns the accumulators run over are saved before the data group is interpolated in place ----
__global__ void accum_gather_kernel(uint32_t* __restrict__ srcvals, const uint32_t* __restrict__ data, Circuit cc) {
    const uint32_t n = 1u << cc.po2;
    const size_t total = (size_t)n * cc.E, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t e = (uint32_t)(i >> cc.po2), r = (uint32_t)(i & (n - 1));
        srcvals[i] = data[(size_t)cc.acc_src(e) * n + r];
    }
}
// run[e][r] = beta_e + x (AoS ext), the input of Hal::prefix_products
__global__ void accum_build_kernel(uint32_t* __restrict__ run, const uint32_t* __restrict__ srcvals, const uint32_t* __restrict__ betas, Circuit cc) {
    const uint32_t n = 1u << cc.po2;
    const size_t total = (size_t)n * cc.E, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t e = (uint32_t)(i >> cc.po2);
        const uint4 b = *reinterpret_cast<const uint4*>(betas + 4 * e);  // wave-uniform
        *reinterpret_cast<uint4*>(run + 4 * i) = make_uint4(fp_add(b.x, srcvals[i]), b.y, b.z, b.w);
    }
}

// ---- eval_check: check(x) = sum_i poly_mix^i C_i(x) / ((3x)^N - 1) on the 4N domain, one thread per domain point ----
template <int TT, int GG>
__global__ __launch_bounds__(256) void eval_check_kernel(uint32_t* __restrict__ check, const uint32_t* __restrict__ ecode,
                                                         const uint32_t* __restrict__ edata, const uint32_t* __restrict__ eacc, Circuit cc,
                                                         const uint32_t* __restrict__ mixpows, const uint32_t* __restrict__ mixpows_c,
                                                         const uint32_t* __restrict__ betas, EvalPoint pt) {
    const uint32_t dom = 4u << cc.po2;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dom) return;
    const uint32_t ib = (i + dom - 4u) & (dom - 1u);   // one row back: x * w_N^-1 = w_4N^(row - 4)
    const uint32_t ib2 = (i + dom - 8u) & (dom - 1u);  // two rows back
    LazyExtAcc mixacc;  // sum_j poly_mix^j * C_j over the derived-column constraints (ext weight x base value)
    mixacc.reset();
    using Regs = DerivedRegs<(TT > 0)>;  // centred registers for the compiled constraint sums, as in witness_derive_kernel
    using word = typename Regs::word;
    const auto code_at = [&](unsigned q) -> word {
        const int col = cc.csel_col(q);
        return Regs::enter(col < 0 ? MONT_ONE : ecode[(size_t)col * dom + i]);
    };
    Regs w;
#pragma unroll
    for (int q = 0; q < 8; ++q) w.ring[q] = code_at((unsigned)q);
#pragma unroll
    for (int q = 0; q < 3; ++q) w.u[q] = Regs::enter(edata[(size_t)((uint32_t)q % cc.F) * dom + i]);
#pragma unroll
    for (int q = 0; q < 4; ++q) w.k[q] = code_at((unsigned)q);
    for (uint32_t j = 0; j < cc.J; ++j) {
        word pool[Circuit::POOL];
        const int sb = Circuit::slot1_back(j);
        w.fill(pool, sb == 0 ? w.u[0] : Regs::enter(edata[(size_t)j * dom + (sb == 1 ? ib : ib2)]));
        const uint32_t d = edata[(size_t)(cc.F + j) * dom + i];  // the committed word: canonical where the constraint subtracts from it
        mix_add(mixacc, mixpows_c, j, fp_sub(d, cons_sum<TT, GG>(pool, cc.T, cc.G)));
        w.shift(Regs::enter(d), Regs::enter(edata[(size_t)((j + 3) % cc.F) * dom + i]), code_at(j + 4));
    }
    // the boundary constraints tying the public words to the trace, first * (data[0] - g0) and last * (data[wd-1] - g1), are base-valued
    // like the walk's: the same accumulator takes them
    const uint32_t first = ecode[i], last = cc.pairs || cc.globals() > 1 ? ecode[(size_t)dom + i] : 0u;
    const size_t b0 = (size_t)cc.J + cc.E + cc.pairs;
    mix_add(mixacc, mixpows_c, b0, fp_mul(first, fp_sub(edata[i], pt.g[0])));
    if (cc.globals() > 1) mix_add(mixacc, mixpows_c, b0 + 1, fp_mul(last, fp_sub(edata[(size_t)(cc.wd - 1) * dom + i], pt.g[1])));
    const Fp4 base = mixacc.finish();
    // the ext-valued constraints are ONE weighted sum: the accumulators' a - inner * fac and the pairs' last * (hi - lo) stay unreduced
    // words (lazy_ext.hpp: accumulator_value, pair_value) and go under their mix powers into seven 64-bit chains that are reduced once
    const TailSelectors sel = tail_selectors(first, last);
    WeightedExtAcc extacc;
    extacc.reset();
    for (uint32_t e = 0; e < cc.E; ++e) {
        Fp4 a, ab;
        ext_column_at(eacc, e, dom, i, ib, a, ab);
        i32 beta[4], v[4];
        uniform_centred(betas, e, true, beta);
        accumulator_value(a, ab, sel, beta, edata[(size_t)cc.acc_src(e) * dom + i], v);
        mix_add(extacc, mixpows_c, cc.J + e, v);
    }
    for (uint32_t p = 0; p < cc.pairs; ++p) {
        Fp4 hi, lo;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            hi.c[k] = eacc[(size_t)(4 * (2 * p + 1) + k) * dom + i];
            lo.c[k] = eacc[(size_t)(4 * (2 * p) + k) * dom + i];
        }
        i32 v[4];
        pair_value(hi, lo, sel, v);
        mix_add(extacc, mixpows_c, cc.J + cc.E + p, v);
    }
    const Fp4 tot = f4_add(base, extacc.finish());
    store_check(check, tot, pt, dom, i);
}

// beta_e = beta^(floor(e/2)+1): the two accumulators of a pair share their challenge
__global__ void beta_table_kernel(uint32_t* __restrict__ out, Fp4 beta, uint32_t n) {
    uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    Fp4 r = f4_pow(beta, e / 2 + 1);
    out[4 * e + 0] = r.c[0]; out[4 * e + 1] = r.c[1]; out[4 * e + 2] = r.c[2]; out[4 * e + 3] = r.c[3];
}
// the statement's public words, read out of the witness
__global__ void globals_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ data, Circuit cc) {
    const size_t n = (size_t)1 << cc.po2;
    if (threadIdx.x == 0) out[0] = data[0];                                  // data[0][0]
    if (threadIdx.x == 1) out[1] = data[(size_t)(cc.wd - 1) * n + (cc.active_rows() - 1)];  // data[wd-1][last active row]
}

// ---------------------------------------------------------------------------------------------------------------------
// the synthetic circuit as a bx_circuit_ops table (include/bx_circuit.h): what bx_prover_create plugs in by default.
// Each entry returns NULL or an error string owned by the ctx; the buffers that arrive through the table are checked against the
// shape, the state's own were sized from it by synth_create.
// ---------------------------------------------------------------------------------------------------------------------
#define BX_CIRCUIT_DISPATCH(KERNEL, ...)                                              \
    do {                                                                              \
        if (cc.T == 64 && cc.G == 4) hipLaunchKernelGGL((KERNEL<64, 4>), __VA_ARGS__); \
        else if (cc.T == 48 && cc.G == 3) hipLaunchKernelGGL((KERNEL<48, 3>), __VA_ARGS__); \
        else if (cc.T == 16 && cc.G == 3) hipLaunchKernelGGL((KERNEL<16, 3>), __VA_ARGS__); \
        else if (cc.T == 8 && cc.G == 2) hipLaunchKernelGGL((KERNEL<8, 2>), __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<0, 0>), __VA_ARGS__);                          \
    } while (0)

namespace {
struct SynthState {
    Circuit cc;
    uint64_t seed = 0;  // of the segment being proved (decoded by witgen from the segment's bytes; accumulate's noise columns use it)
    NoiseSeed noise;
    // perm_offsets / perm_index: the scatters of the permuted copies (built once); acc_src: the columns the accumulators run over;
    // acc_run: E AoS ext runs; betas: the accumulators' challenges; mixpows: eval_check's weights (canonical table + centred copy)
    DevBuf perm_offsets, perm_index, acc_src, acc_run, betas, mixpows;
};
void synth_destroy(void*, void* state) { delete (SynthState*)state; }
const char* synth_create(void*, bx_ctx* c, const bx_segment_params* shape, void** state) {
    std::unique_ptr<SynthState> st(new (std::nothrow) SynthState());
    BX_REQUIRE(c, st != nullptr, "synthetic circuit: out of host memory");
    st->cc = circuit_of(shape);
    const Circuit& cc = st->cc;
    const size_t n = (size_t)1 << cc.po2;
    BX_TRY(st->mixpows.alloc(c, 8 * (cc.constraints() + 1)));
    BX_TRY(st->perm_offsets.alloc(c, n * (cc.pairs ? cc.pairs : 1)));
    BX_TRY(st->perm_index.alloc(c, n + 1));
    BX_TRY(st->acc_src.alloc(c, n * (cc.E ? cc.E : 1)));
    BX_TRY(st->acc_run.alloc(c, 4 * n * (cc.E ? cc.E : 1)));
    BX_TRY(st->betas.alloc(c, 4 * (cc.E ? cc.E : 1)));
    hipLaunchKernelGGL(perm_offsets_kernel, dim3(grid_for(n * (cc.pairs ? cc.pairs : 1))), dim3(256), 0, c->stream, (uint32_t*)st->perm_offsets.b.dptr,
                       (uint32_t*)st->perm_index.b.dptr, cc);
    BX_LAUNCH_CHECK(c);
    *state = st.release();
    return nullptr;
}
// the code group (public; what bx_prover_control_id commits)
const char* synth_code_group(void*, void* state, bx_ctx* c, bx_buf code) {
    const Circuit& cc = ((SynthState*)state)->cc;
    const size_t n = (size_t)1 << cc.po2;
    BX_REQUIRE(c, code.len == n * cc.wc, "circuit_code: group buffer size mismatch");
    OpScope op(c, "witgen_code", 4.0 * (double)(n * cc.wc));
    hipLaunchKernelGGL(witness_code_kernel, dim3(grid_for(n * cc.wc)), dim3(256), 0, c->stream, (uint32_t*)code.dptr, cc);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
// The synthetic segment is "BXSYNSEG" | index | po2 | seed | payload (bx_prover.h): the witness is a function of the seed; the
// payload stands for the preflight trace (it is uploaded like one: `segment_dev`) and is not read.
// `data`/`code` are the groups' column-major N x width buffers (code already filled); the permuted copies go through Hal::scatter
// (one call per pair, one entry per cycle), the derived columns through one thread per row.
const char* synth_witgen(void*, void* state, bx_ctx* c, bx_buf code, bx_buf data, const uint8_t* segment, size_t segment_len, bx_buf /*segment_dev*/,
                         uint32_t* globals_out) {
    auto* st = (SynthState*)state;
    const Circuit& cc = st->cc;
    const size_t n = (size_t)1 << cc.po2;
    uint64_t seed = 0;
    const char* refused = segment_header(c, segment, segment_len, cc.po2, &seed);
    const uint64_t noise = st->noise.take(seed);  // the ZK rows' generator (bx_prover.h, "seeds"): this witgen's, accepted or refused
    if (refused) return refused;
    BX_REQUIRE(c, code.len == n * cc.wc && data.len == n * cc.wd, "circuit_witness: group buffer size mismatch");
    st->seed = seed;
    {
        OpScope op(c, "witgen_fill", 4.0 * (double)(n * cc.F));
        hipLaunchKernelGGL(witness_free_kernel, dim3(grid_for(n * cc.F)), dim3(256), 0, c->stream, (uint32_t*)data.dptr, cc, data_seed(seed),
                           data_seed(noise));
        BX_LAUNCH_CHECK(c);
    }
    for (uint32_t p = 0; p < cc.pairs; ++p) {
        bx_buf values{(uint32_t*)data.dptr + (size_t)(4 * p + 2) * n, n}, into{(uint32_t*)data.dptr + (size_t)(4 * p + 3) * n, n};
        BX_TRY(bx_scatter(c, into, st->perm_index.slice(0, n + 1), st->perm_offsets.slice((size_t)p * n, n), values));
    }
    if (cc.J) {
        OpScope op(c, "witgen_derive", 4.0 * (double)(n * (cc.J + cc.J + cc.J / 4)));
        BX_CIRCUIT_DISPATCH(witness_derive_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (uint32_t*)data.dptr,
                            (const uint32_t*)code.dptr, cc);
        BX_LAUNCH_CHECK(c);
    }
    if (cc.E) {  // the prover interpolates `data` in place next
        OpScope op(c, "accum_gather", 8.0 * (double)(n * cc.E));
        hipLaunchKernelGGL(accum_gather_kernel, dim3(grid_for(n * cc.E)), dim3(256), 0, c->stream, (uint32_t*)st->acc_src.b.dptr,
                           (const uint32_t*)data.dptr, cc);
        BX_LAUNCH_CHECK(c);
    }
    // the statement's public words come out of the witness (one small copy; the derived cell is only known on the device)
    hipLaunchKernelGGL(globals_kernel, dim3(1), dim3(64), 0, c->stream, (uint32_t*)st->betas.b.dptr, (const uint32_t*)data.dptr, cc);
    BX_LAUNCH_CHECK(c);
    uint32_t g[2] = {0, 0};
    BX_TRY(bx_d2h(c, g, st->betas.slice(0, 2), 2));  // betas is written by accumulate later: free to borrow here
    for (uint32_t i = 0; i < cc.globals(); ++i) globals_out[i] = g[i];
    return nullptr;
}
void synth_set_noise_seed(void*, void* state, uint64_t noise_seed) { ((SynthState*)state)->noise.set(noise_seed); }
const char* synth_betas(bx_ctx* c, SynthState* st, const uint32_t mix[4]) {
    if (!st->cc.E) return nullptr;
    hipLaunchKernelGGL(beta_table_kernel, dim3((st->cc.E + 63) / 64), dim3(64), 0, c->stream, (uint32_t*)st->betas.b.dptr,
                       Fp4{{mix[0], mix[1], mix[2], mix[3]}}, st->cc.E);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
// the accumulate step: run = beta_e + x  ->  Hal::prefix_products  ->  accum columns (+ noise columns)
const char* synth_accumulate(void*, void* state, bx_ctx* c, bx_buf accum, const uint32_t mix[4]) {
    auto* st = (SynthState*)state;
    const Circuit& cc = st->cc;
    const size_t n = (size_t)1 << cc.po2;
    BX_REQUIRE(c, accum.len == n * cc.wa, "circuit_accumulate: group buffer size mismatch");
    BX_TRY(synth_betas(c, st, mix));
    if (cc.E) {
        {
            OpScope op(c, "accum_build", 20.0 * (double)(n * cc.E));
            hipLaunchKernelGGL(accum_build_kernel, dim3(grid_for(n * cc.E)), dim3(256), 0, c->stream, (uint32_t*)st->acc_run.b.dptr,
                               (const uint32_t*)st->acc_src.b.dptr, (const uint32_t*)st->betas.b.dptr, cc);
            BX_LAUNCH_CHECK(c);
        }
        BX_TRY(bx_batch_prefix_products(c, st->acc_run.slice(0, 4 * n * cc.E), cc.E));
    }
    OpScope op(c, "accum_store", 4.0 * (double)(n * cc.wa) + 16.0 * (double)(n * cc.E));
    return store_ext_columns(c, accum, st->acc_run.b, cc.po2, cc.E, cc.wa, filler_seed(st->seed, mix));
}
// eval_check over the committed 4N evaluations; `check` receives the four ext planes of check(x) over the domain
const char* synth_eval_check(void*, void* state, bx_ctx* c, bx_buf check, bx_buf ecode, bx_buf edata, bx_buf eacc, const uint32_t poly_mix[4],
                             const uint32_t mix[4], const uint32_t* globals) {
    auto* st = (SynthState*)state;
    const Circuit& cc = st->cc;
    const size_t dom = (size_t)4 << cc.po2;
    BX_REQUIRE(c, check.len == 4 * dom && ecode.len == dom * cc.wc && edata.len == dom * cc.wd && eacc.len == dom * cc.wa,
               "circuit_eval_check: buffer size mismatch");
    BX_TRY(synth_betas(c, st, mix));
    BX_TRY(mix_power_table(c, st->mixpows.b, poly_mix, (uint32_t)cc.constraints()));
    EvalPoint pt;
    vanishing_inverses(cc.po2, pt.zinv);
    pt.g[0] = globals[0];
    pt.g[1] = cc.globals() > 1 ? globals[1] : 0u;
    // every committed evaluation is read once (plus the one-row-back taps), the check planes are written once
    OpScope op(c, "eval_check", 4.0 * (double)dom * (cc.wc + cc.wd + cc.J / 4.0 + 2.0 * cc.wa + 4.0));
    BX_CIRCUIT_DISPATCH(eval_check_kernel, dim3((unsigned)((dom + 255) / 256)), dim3(256), 0, c->stream, (uint32_t*)check.dptr,
                        (const uint32_t*)ecode.dptr, (const uint32_t*)edata.dptr, (const uint32_t*)eacc.dptr, cc, (const uint32_t*)st->mixpows.b.dptr,
                        (const uint32_t*)st->mixpows.b.dptr + 4 * cc.constraints(), (const uint32_t*)st->betas.b.dptr, pt);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
}  // namespace

}  // namespace bx

extern "C" const bx_circuit_ops* bx_synthetic_circuit(void) {
    static const bx_circuit_ops ops = {nullptr,
                                       "bx-synthetic-air",
                                       bx::synth_normalize,
                                       bx::synth_taps,
                                       bx::synth_n_globals,
                                       bx::synth_create,
                                       bx::synth_destroy,
                                       bx::synth_code_group,
                                       bx::synth_witgen,
                                       bx::synth_accumulate,
                                       bx::synth_eval_check,
                                       bx::synthetic_constraints_at,
                                       bx::synth_set_noise_seed,
                                       bx::synth_check_code};
    return &ops;
}
