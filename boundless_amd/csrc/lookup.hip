// lookup.hip — device side of the lookup circuit (include/bx_lookup.h, "The lookup circuit", is the normative text; lookup.hpp holds
// the shape rules shared with the host verifier): a range check of V values, two limbs each, proved with LogUp running sums.
//   witgen      cells from the seed, the segment's cell records on top, then the multiplicity HISTOGRAM of the 2V limb columns
//   accumulate  denominators alpha - a_s(r) and the table's multiplicities -> ONE bx_logup_accumulate over 2V + 1 sequences -> the
//               AoS ext sums transposed into 4 (2V + 1) base columns
//   eval_check  the 3V + 4 constraints over the 4N domain, divided by the vanishing polynomial
// The histogram is the one stage with contention: half of the hi limbs are zero by construction, so about V/2 * A of the 2V * A
// increments hit bin 0.  One global atomic per limb serialises on that bin in L2.  The table is at most 2^15 bins = 128 KiB, which
// fits the 160 KiB of LDS of a CDNA4 workgroup: lookup_hist_lds_kernel counts into per-workgroup LDS bins — the lanes of a wave that
// hit the first live lane's bin are counted with one ballot and added by one lane, as msm_bucket_kernel (bn254.hip) does, which
// turns a constant column into one LDS atomic per wave — and flushes every non-zero bin with one global atomic.  ctx tunable
// lookup_hist_lds = 0 keeps the plain form for comparison (tools/lookup_bench.py); both give the same counts.
// eval_check costs one ext x ext product per sequence and domain point (f4_mul_lz, lazy_ext.hpp) and the 16 raw products that take its
// constraint into the weighted sum (WeightedExtAcc, reduced once per point), and is VALU-bound like the
// synthetic circuit's; everything else here streams.
#define BX_PLAIN_MAD 1
#include <memory>
#include <new>
#include <unordered_map>
#include <vector>

#include "circuit_common.hpp"
#include "lookup.hpp"

namespace bx {

// ---- witness: code group (first, last, the table, control words) ----
__global__ void lookup_code_kernel(uint32_t* __restrict__ code, Lookup lk) {
    const uint32_t n = 1u << lk.po2;
    const size_t total = (size_t)n * lk.wc, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
        code[i] = lookup_code_cell(lk, (uint32_t)(i >> lk.po2), (uint32_t)(i & (n - 1)));
}

// ---- witness: every data cell but the active rows of the multiplicity column (lookup_mult_kernel) ----
__global__ void lookup_fill_kernel(uint32_t* __restrict__ data, Lookup lk, uint64_t gseed, uint64_t nseed) {
    const uint32_t n = 1u << lk.po2, act = lk.active_rows(), mask = lk.B - 1u;
    const uint32_t mont_b = fp_mul(R2, lk.B);
    const size_t total = (size_t)n * lk.wd, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t c = (uint32_t)(i >> lk.po2), r = (uint32_t)(i & (n - 1));
        const bool triple = c < 3 * lk.V;
        const uint32_t j = c / 3, k = c - 3 * j;
        uint32_t cell;
        if (r >= act) {  // noise rows: the limbs are noise, v_j follows them so that v = lo + B hi holds on every row
            cell = (triple && k == 0) ? fp_add(synth_word(nseed, c + 1, r), fp_mul(mont_b, synth_word(nseed, c + 2, r))) : synth_word(nseed, c, r);
        } else if (triple) {
            const uint32_t lo = synth_word(gseed, 3 * j + 1, r) & mask;
            const uint32_t hi = (j & 1u) ? 0u : synth_word(gseed, 3 * j + 2, r) & mask;
            cell = fp_mul(R2, k == 0 ? lo + lk.B * hi : (k == 1 ? lo : hi));  // < 2^30: the value's Montgomery word
        } else if (c == lk.mult_col()) {
            cell = 0u;
        } else {
            cell = synth_word(gseed, c, r);
        }
        data[i] = cell;
    }
}
// the segment's cell records, made unique on the host (the last record of a cell wins): rec = (col, row, Montgomery word)
__global__ void lookup_records_kernel(uint32_t* __restrict__ data, const uint32_t* __restrict__ rec, uint32_t count, Lookup lk) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const uint32_t col = rec[3 * k], row = rec[3 * k + 1];
    if (col < 3 * lk.V && row < lk.active_rows()) data[((size_t)col << lk.po2) + row] = rec[3 * k + 2];
}
// the limb columns are kept for the histogram and for accumulate (the prover interpolates `data` in place after witgen)
__global__ void lookup_gather_kernel(uint32_t* __restrict__ limbs, const uint32_t* __restrict__ data, Lookup lk) {
    const uint32_t n = 1u << lk.po2;
    const size_t total = (size_t)n * 2 * lk.V, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
        limbs[i] = data[((size_t)lk.limb_col((uint32_t)(i >> lk.po2)) << lk.po2) + (i & (n - 1))];
}

// ---- the multiplicity histogram over limbs[2V][N], active rows only; a limb that holds no value below B is not counted ----
constexpr int HIST_T = 1024;
__global__ __launch_bounds__(HIST_T) void lookup_hist_lds_kernel(uint32_t* __restrict__ counts, const uint32_t* __restrict__ limbs, Lookup lk,
                                                                 size_t total, size_t per_wg) {
    extern __shared__ uint32_t bins[];  // lk.B words
    const uint32_t n = 1u << lk.po2, act = lk.active_rows();
    for (uint32_t b = threadIdx.x; b < lk.B; b += HIST_T) bins[b] = 0u;
    __syncthreads();
    const size_t begin = (size_t)blockIdx.x * per_wg, end = begin + per_wg < total ? begin + per_wg : total;
    const uint32_t lane = __lane_id();
    for (size_t base = begin; base < end; base += HIST_T) {  // the same trip count for every lane: whole waves reach the ballots
        const size_t i = base + threadIdx.x;
        uint32_t v = lk.B;
        if (i < end && (uint32_t)(i & (n - 1)) < act) v = fp_decode(limbs[i]);
        const bool live = v < lk.B;
        const uint64_t any = __ballot(live);
        if (!any) continue;
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)any) - 1;
        const uint32_t lb = __shfl(v, (int)leader);
        const bool peer = live && v == lb;
        const uint64_t peers = __ballot(peer);
        if (lane == leader) atomicAdd(&bins[lb], (uint32_t)__popcll(peers));
        else if (live && !peer) atomicAdd(&bins[v], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < lk.B; b += HIST_T) {
        const uint32_t cnt = bins[b];
        if (cnt) atomicAdd(&counts[b], cnt);
    }
}
__global__ void lookup_hist_atomic_kernel(uint32_t* __restrict__ counts, const uint32_t* __restrict__ limbs, Lookup lk, size_t total) {
    const uint32_t n = 1u << lk.po2, act = lk.active_rows();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        if ((uint32_t)(i & (n - 1)) >= act) continue;
        const uint32_t v = fp_decode(limbs[i]);
        if (v < lk.B) atomicAdd(&counts[v], 1u);
    }
}
// m(r) into the data group's active rows, and the whole column (noise rows included) into the state for accumulate
__global__ void lookup_mult_kernel(uint32_t* __restrict__ data, uint32_t* __restrict__ mcol, const uint32_t* __restrict__ counts, Lookup lk) {
    const uint32_t n = 1u << lk.po2, r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    uint32_t* cell = data + ((size_t)lk.mult_col() << lk.po2) + r;
    if (r < lk.active_rows()) *cell = r < lk.B ? fp_mul(R2, counts[r] % P) : 0u;
    mcol[r] = *cell;
}

// ---- accumulate: denominators alpha - a_s(r) (AoS ext) and the table's multiplicities -m(r); mults of the limb sequences stay 1 ----
__global__ void lookup_build_kernel(uint32_t* __restrict__ denoms, uint32_t* __restrict__ mults, const uint32_t* __restrict__ limbs,
                                    const uint32_t* __restrict__ mcol, Lookup lk, Fp4 alpha) {
    const uint32_t n = 1u << lk.po2;
    const size_t total = (size_t)n * lk.S, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t s = (uint32_t)(i >> lk.po2), r = (uint32_t)(i & (n - 1));
        uint32_t a;
        if (s < 2 * lk.V) {
            a = limbs[i];
        } else {
            a = r < lk.B ? fp_mul(R2, r) : 0u;  // t(r)
            mults[i] = fp_neg(mcol[r]);
        }
        *reinterpret_cast<uint4*>(denoms + 4 * i) = make_uint4(fp_sub(alpha.c[0], a), alpha.c[1], alpha.c[2], alpha.c[3]);
    }
}

// ---- eval_check: sum_i poly_mix^i C_i(x) / ((3x)^N - 1) on the 4N domain, one thread per domain point ----
struct LookupPoint {
    EvalPoint at;
    uint32_t mont_b;  // B
    Fp4 alpha;
};
__global__ __launch_bounds__(256) void lookup_eval_check_kernel(uint32_t* __restrict__ check, const uint32_t* __restrict__ ecode,
                                                                const uint32_t* __restrict__ edata, const uint32_t* __restrict__ eacc, Lookup lk,
                                                                const uint32_t* __restrict__ mixpows, const uint32_t* __restrict__ mixpows_c,
                                                                LookupPoint pt) {
    const uint32_t dom = 4u << lk.po2;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dom) return;
    const uint32_t ib = (i + dom - 4u) & (dom - 1u);  // one row back: x * w_N^-1 = w_4N^(row - 4)
    const uint32_t first = ecode[i], last = ecode[(size_t)dom + i], table = ecode[2 * (size_t)dom + i];
    const uint32_t not_first = fp_sub(MONT_ONE, first);
    // (S_s(x) - (1 - first) S_s(x w_N^-1)) * (alpha - a) + add, weighted poly_mix^(V + s); returns S_s(x) for the closing sum.  The
    // ext-valued constraints are one weighted sum (lazy_ext.hpp, WeightedExtAcc): a canonical value goes in as it is, under the centred
    // mix power, and the sum is reduced once
    WeightedExtAcc extacc;
    extacc.reset();
    Fp4 closing = f4_zero();
    const auto mix_ext = [&](size_t k, const Fp4& val) {
        const i32 v[4] = {(i32)val.c[0], (i32)val.c[1], (i32)val.c[2], (i32)val.c[3]};
        mix_add(extacc, mixpows_c, k, v);
    };
    const auto sequence = [&](uint32_t s, uint32_t a, const Fp4& add) {
        Fp4 cur, back;
        ext_column_at(eacc, s, dom, i, ib, cur, back);
        const Fp4 step = f4_sub(cur, f4_scale(back, not_first));
        const Fp4 den{{fp_sub(pt.alpha.c[0], a), pt.alpha.c[1], pt.alpha.c[2], pt.alpha.c[3]}};
        mix_ext(lk.V + s, f4_add(f4_mul_lz(step, den), add));
        closing = f4_add(closing, cur);
    };
    LazyExtAcc mixacc;  // the base-valued constraints: v - lo - B hi, and the two boundary ones
    mixacc.reset();
    const Fp4 minus_one{{fp_neg(MONT_ONE), 0u, 0u, 0u}};
    for (uint32_t j = 0; j < lk.V; ++j) {
        const uint32_t v = edata[(size_t)(3 * j) * dom + i], lo = edata[(size_t)(3 * j + 1) * dom + i], hi = edata[(size_t)(3 * j + 2) * dom + i];
        mix_add(mixacc, mixpows_c, j, fp_sub(fp_sub(v, lo), fp_mul(pt.mont_b, hi)));
        sequence(2 * j, lo, minus_one);
        sequence(2 * j + 1, hi, minus_one);
    }
    sequence(2 * lk.V, table, Fp4{{edata[(size_t)lk.mult_col() * dom + i], 0u, 0u, 0u}});
    const size_t k0 = 3 * (size_t)lk.V + 1;
    mix_ext(k0, f4_scale(closing, last));
    const uint32_t v0 = edata[i];
    mix_add(mixacc, mixpows_c, k0 + 1, fp_mul(first, fp_sub(v0, pt.at.g[0])));
    mix_add(mixacc, mixpows_c, k0 + 2, fp_mul(last, fp_sub(v0, pt.at.g[1])));
    const Fp4 tot = f4_add(mixacc.finish(), extacc.finish());
    store_check(check, tot, pt.at, dom, i);
}

// ---------------------------------------------------------------------------------------------------------------------
// the lookup circuit as a bx_circuit_ops table (include/bx_circuit.h)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct LookupState {
    Lookup lk;
    uint64_t seed = 0;
    NoiseSeed noise;
    // limbs: the 2V limb columns; mcol: the multiplicity column; counts: B bins; run: S AoS ext sequences (denominators, then sums);
    // mults: S sequences of multiplicities; records: the segment's cell records; mixpows: eval_check's weights
    DevBuf limbs, mcol, counts, run, mults, records, mixpows;
};
void lookup_destroy(void*, void* state) { delete (LookupState*)state; }
__global__ void fill_words_kernel(uint32_t* __restrict__ out, uint32_t value, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = value;
}
const char* lookup_create(void*, bx_ctx* c, const bx_segment_params* shape, void** state) {
    bx_segment_params checked = *shape;  // the prover normalised it already; a direct caller of the table may not have
    if (const char* e = lookup_normalize(nullptr, &checked)) return set_msg(c, e);
    std::unique_ptr<LookupState> st(new (std::nothrow) LookupState());
    BX_REQUIRE(c, st != nullptr, "lookup circuit: out of host memory");
    st->lk = lookup_of(shape);
    const Lookup& lk = st->lk;
    const size_t n = (size_t)1 << lk.po2;
    BX_TRY(st->mixpows.alloc(c, 8 * (lk.constraints() + 1)));
    BX_TRY(st->limbs.alloc(c, n * 2 * lk.V));
    BX_TRY(st->mcol.alloc(c, n));
    BX_TRY(st->counts.alloc(c, lk.B));
    BX_TRY(st->run.alloc(c, 4 * n * lk.S));
    BX_TRY(st->mults.alloc(c, n * lk.S));
    BX_TRY(st->records.alloc(c, 3 * (size_t)BX_LOOKUP_MAX_RECORDS));
    // a table of 2^15 bins needs more dynamic LDS than a kernel may use by default (set once per process and kernel; cheap to repeat)
    BX_REQUIRE(c, (size_t)lk.B * 4 <= 64 * 1024 ||
                      hipFuncSetAttribute((const void*)lookup_hist_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lk.B * 4)) == hipSuccess,
               "lookup circuit: the histogram's LDS bins could not be reserved");
    // every limb is looked up once: the multiplicities of the 2V limb sequences are the constant 1
    hipLaunchKernelGGL(fill_words_kernel, dim3(grid_for(n * 2 * lk.V)), dim3(256), 0, c->stream, (uint32_t*)st->mults.b.dptr, MONT_ONE, n * 2 * lk.V);
    BX_REQUIRE(c, hipGetLastError() == hipSuccess, "lookup circuit: launch failed");
    *state = st.release();
    return nullptr;
}
const char* lookup_code_group(void*, void* state, bx_ctx* c, bx_buf code) {
    const Lookup& lk = ((LookupState*)state)->lk;
    const size_t n = (size_t)1 << lk.po2;
    BX_REQUIRE(c, code.len == n * lk.wc, "lookup circuit: code group buffer size mismatch");
    OpScope op(c, "lookup_code", 4.0 * (double)(n * lk.wc));
    hipLaunchKernelGGL(lookup_code_kernel, dim3(grid_for(n * lk.wc)), dim3(256), 0, c->stream, (uint32_t*)code.dptr, lk);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
void lookup_set_noise_seed(void*, void* state, uint64_t noise_seed) { ((LookupState*)state)->noise.set(noise_seed); }

const char* lookup_histogram(bx_ctx* c, LookupState* st) {
    const Lookup& lk = st->lk;
    const size_t total = ((size_t)2 * lk.V) << lk.po2;
    BX_HIP(c, hipMemsetAsync(st->counts.b.dptr, 0, (size_t)lk.B * 4, c->stream));
    OpScope op(c, "lookup_hist", 4.0 * (double)total);  // the histogram kernel alone
    if (c->lookup_hist_lds) {
        const size_t lds = (size_t)lk.B * 4;
        // one workgroup per CU (a 128 KiB table leaves room for no second one), at least 8 limbs per lane
        size_t wgs = (total + 8 * HIST_T - 1) / (8 * HIST_T);
        if (wgs > (size_t)c->cu_count) wgs = (size_t)c->cu_count;
        const size_t per_wg = ((total + wgs - 1) / wgs + HIST_T - 1) / HIST_T * HIST_T;
        hipLaunchKernelGGL(lookup_hist_lds_kernel, dim3((unsigned)wgs), dim3(HIST_T), lds, c->stream, (uint32_t*)st->counts.b.dptr,
                           (const uint32_t*)st->limbs.b.dptr, lk, total, per_wg);
    } else {
        hipLaunchKernelGGL(lookup_hist_atomic_kernel, dim3(grid_for(total)), dim3(256), 0, c->stream, (uint32_t*)st->counts.b.dptr,
                           (const uint32_t*)st->limbs.b.dptr, lk, total);
    }
    BX_LAUNCH_CHECK(c);
    return nullptr;
}

// The segment is "BXSYNSEG" | index | po2 | seed | cell records (bx_lookup.h, "segment"): parsed from the host copy, made unique
// (the last record of a cell wins) and uploaded through the pinned ring; the HBM copy of the segment is not needed.
const char* lookup_witgen_impl(LookupState* st, bx_ctx* c, bx_buf data, const uint8_t* segment, size_t segment_len, uint32_t* globals_out) {
    const Lookup& lk = st->lk;
    const size_t n = (size_t)1 << lk.po2;
    const uint32_t act = lk.active_rows();
    uint64_t seed = 0;
    const char* refused = segment_header(c, segment, segment_len, lk.po2, &seed);
    const uint64_t noise = st->noise.take(seed);  // a noise seed given through set_noise_seed belongs to THIS witgen, accepted or refused
    if (refused) return refused;
    BX_REQUIRE(c, data.len == n * lk.wd, "lookup witgen: data group buffer size mismatch");
    const uint8_t* payload = segment + BX_SEGMENT_WIRE_BYTES;
    const size_t payload_len = segment_len - BX_SEGMENT_WIRE_BYTES;
    BX_REQUIRE(c, payload_len % BX_LOOKUP_RECORD_BYTES == 0, "lookup witgen: the payload is not a whole number of 12-byte cell records");
    const size_t n_rec = payload_len / BX_LOOKUP_RECORD_BYTES;
    BX_REQUIRE(c, n_rec <= BX_LOOKUP_MAX_RECORDS, "lookup witgen: more than 65536 cell records");
    std::vector<uint32_t> recs;
    std::unordered_map<uint64_t, size_t> where;  // cell -> its record in recs
    for (size_t k = 0; k < n_rec; ++k) {
        uint32_t w[3];
        for (int q = 0; q < 3; ++q) {
            const uint8_t* p = payload + BX_LOOKUP_RECORD_BYTES * k + 4 * q;
            w[q] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
        if (w[0] >= 3 * lk.V || w[1] >= act || w[2] >= P) {
            snprintf(c->err, sizeof c->err, "lookup witgen: cell record %zu (col %u, row %u, value %u) is out of bounds: col < %u, row < %u and value < P are needed",
                     k, w[0], w[1], w[2], 3 * lk.V, act);
            return c->err;
        }
        const auto ins = where.emplace(((uint64_t)w[0] << 32) | w[1], recs.size() / 3);
        if (ins.second) recs.insert(recs.end(), {w[0], w[1], 0u});
        recs[3 * ins.first->second + 2] = fp_encode(w[2]);
    }
    st->seed = seed;
    const uint64_t gseed = data_seed(seed), nseed = data_seed(noise);
    // the statement's public words v_0[0], v_0[A-1]: a generated cell, or the record that replaced it
    for (int q = 0; q < 2; ++q) {
        const uint32_t r = q ? act - 1 : 0u;
        const auto it = where.find((uint64_t)r);  // column 0
        globals_out[q] = it != where.end() ? recs[3 * it->second + 2]
                                           : fp_encode((synth_word(gseed, 1, r) & (lk.B - 1u)) + lk.B * (synth_word(gseed, 2, r) & (lk.B - 1u)));
    }
    const uint32_t count = (uint32_t)(recs.size() / 3);
    if (count) BX_TRY(h2d_staged(c, bx_buf{st->records.b.dptr, recs.size()}, recs.data(), recs.size()));
    {
        OpScope op(c, "lookup_fill", 4.0 * (double)(n * lk.wd) + 8.0 * (double)(n * 2 * lk.V));
        hipLaunchKernelGGL(lookup_fill_kernel, dim3(grid_for(n * lk.wd)), dim3(256), 0, c->stream, (uint32_t*)data.dptr, lk, gseed, nseed);
        BX_LAUNCH_CHECK(c);
        if (count) {
            hipLaunchKernelGGL(lookup_records_kernel, dim3((count + 255) / 256), dim3(256), 0, c->stream, (uint32_t*)data.dptr,
                               (const uint32_t*)st->records.b.dptr, count, lk);
            BX_LAUNCH_CHECK(c);
        }
        hipLaunchKernelGGL(lookup_gather_kernel, dim3(grid_for(n * 2 * lk.V)), dim3(256), 0, c->stream, (uint32_t*)st->limbs.b.dptr,
                           (const uint32_t*)data.dptr, lk);
        BX_LAUNCH_CHECK(c);
    }
    BX_TRY(lookup_histogram(c, st));
    OpScope op(c, "lookup_mult", 12.0 * (double)n);
    hipLaunchKernelGGL(lookup_mult_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (uint32_t*)data.dptr, (uint32_t*)st->mcol.b.dptr,
                       (const uint32_t*)st->counts.b.dptr, lk);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}

// no exception crosses the table: the record list lives in host containers
const char* lookup_witgen(void*, void* state, bx_ctx* c, bx_buf /*code*/, bx_buf data, const uint8_t* segment, size_t segment_len, bx_buf /*segment_dev*/,
                          uint32_t* globals_out) try {
    return lookup_witgen_impl((LookupState*)state, c, data, segment, segment_len, globals_out);
} catch (...) {
    return set_msg(c, "lookup witgen: out of host memory");
}

const char* lookup_accumulate(void*, void* state, bx_ctx* c, bx_buf accum, const uint32_t mix[4]) {
    auto* st = (LookupState*)state;
    const Lookup& lk = st->lk;
    const size_t n = (size_t)1 << lk.po2;
    BX_REQUIRE(c, accum.len == n * lk.wa, "lookup accumulate: accum group buffer size mismatch");
    {
        OpScope op(c, "lookup_build", 24.0 * (double)(n * lk.S));
        hipLaunchKernelGGL(lookup_build_kernel, dim3(grid_for(n * lk.S)), dim3(256), 0, c->stream, (uint32_t*)st->run.b.dptr, (uint32_t*)st->mults.b.dptr,
                           (const uint32_t*)st->limbs.b.dptr, (const uint32_t*)st->mcol.b.dptr, lk, Fp4{{mix[0], mix[1], mix[2], mix[3]}});
        BX_LAUNCH_CHECK(c);
    }
    BX_TRY(bx_logup_accumulate(c, st->run.b, st->run.b, st->mults.b, lk.S));  // in place: the sums replace the denominators
    OpScope op(c, "lookup_store", 4.0 * (double)(n * lk.wa) + 16.0 * (double)(n * lk.S));
    return store_ext_columns(c, accum, st->run.b, lk.po2, lk.S, lk.wa, filler_seed(st->seed, mix));
}

const char* lookup_eval_check(void*, void* state, bx_ctx* c, bx_buf check, bx_buf ecode, bx_buf edata, bx_buf eacc, const uint32_t poly_mix[4],
                              const uint32_t mix[4], const uint32_t* globals) {
    auto* st = (LookupState*)state;
    const Lookup& lk = st->lk;
    const size_t dom = (size_t)4 << lk.po2;
    BX_REQUIRE(c, check.len == 4 * dom && ecode.len == dom * lk.wc && edata.len == dom * lk.wd && eacc.len == dom * lk.wa,
               "lookup eval_check: buffer size mismatch");
    BX_TRY(mix_power_table(c, st->mixpows.b, poly_mix, (uint32_t)lk.constraints()));
    LookupPoint pt;
    vanishing_inverses(lk.po2, pt.at.zinv);
    pt.at.g[0] = globals[0];
    pt.at.g[1] = globals[1];
    pt.mont_b = fp_encode(lk.B);
    pt.alpha = Fp4{{mix[0], mix[1], mix[2], mix[3]}};
    // every evaluation the constraints name is read once, the running sums twice (the tap one row back); four planes are written
    OpScope op(c, "lookup_eval_check", 4.0 * (double)dom * (3.0 + 3.0 * lk.V + 1.0 + 8.0 * lk.S + 4.0));
    hipLaunchKernelGGL(lookup_eval_check_kernel, dim3((unsigned)((dom + 255) / 256)), dim3(256), 0, c->stream, (uint32_t*)check.dptr,
                       (const uint32_t*)ecode.dptr, (const uint32_t*)edata.dptr, (const uint32_t*)eacc.dptr, lk, (const uint32_t*)st->mixpows.b.dptr,
                       (const uint32_t*)st->mixpows.b.dptr + 4 * lk.constraints(), pt);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
}  // namespace
}  // namespace bx

extern "C" const bx_circuit_ops* bx_lookup_circuit(void) {
    static const bx_circuit_ops ops = {nullptr,
                                       "bx-lookup-logup",
                                       bx::lookup_normalize,
                                       bx::lookup_taps,
                                       bx::lookup_n_globals,
                                       bx::lookup_create,
                                       bx::lookup_destroy,
                                       bx::lookup_code_group,
                                       bx::lookup_witgen,
                                       bx::lookup_accumulate,
                                       bx::lookup_eval_check,
                                       bx::lookup_constraints_at,
                                       bx::lookup_set_noise_seed,
                                       bx::lookup_check_code};
    return &ops;
}
