// scan.hip — every scan over AoS ext arrays for gfx950: the DEEP quotient (poly_divide*), prefix_products, prefix_sums, the
// additive half of an accumulate stage (batch inversion, logup_accumulate), and the running product of ratios (batch_ratio_products).
//
// Restates risc0_zkp::core::poly::poly_divide (run once per tap point of every DEEP combination polynomial by
// Prover::finalize) and risc0_zkp::hal::Hal::prefix_products (risc0-zkp 3.0.3, reference Cargo.lock:9155), reached from
// bento/crates/workflow/src/tasks/prove.rs:41-49.
//
// All are first-order recurrences over 16-byte elements whose algorithmic traffic is one read and one write of the array.  Each has
// two forms, and every entry point reads the same way: validate, open the OpScope, then "look-back if enabled (the scan_lookback
// tunable) and 16-byte aligned, else three-phase".
//
// LOOK-BACK, the default: ONE launch.  A workgroup owns a tile of 2048 elements (loaded coalesced, transposed through LDS so that a
// lane owns 8 consecutive elements), scans it in registers and wave shuffles, publishes its aggregate, and obtains the carry entering
// the tile by DECOUPLED LOOK-BACK: wave 0 inspects the 64 preceding tiles at once, takes the nearest published inclusive value and
// the aggregates after it, and moves on 64 tiles at a time until it finds one.  Tiles are handed out by a ticket counter, so a
// tile's predecessors are always running or finished and the spin terminates.  Each array is read once and written once.
// The tile load, the tile store and the look-back loop are written once (sc_tile_load, sc_tile_store, sc_look_back); products, sums
// and the fused LogUp sum are one kernel over an operator (ScanMul, ScanSum); the division keeps its own body between the shared pieces.
//
// Publication protocol.  An ext value is four words < 2^31, so bit 31 of every word is free: a slot is written with four
// relaxed agent-scope atomic stores of (word | 2^31) and read with four relaxed agent-scope atomic loads; the value is taken
// only when all four words carry the bit.  Every word validates itself, so no ordering between the four is needed and a torn
// read is simply retried.  Slots must start at zero: the state lives in two alternating buffers, and every launch clears the
// extent the OTHER buffer was last used with (calls on a ctx are stream-ordered), so no memset launch is ever needed.
//
// poly_divide specifics: the recurrence runs from the top coefficient down, cur <- z cur + p_i with out_i = cur before the
// update; an element's map is affine with a known slope (z), so a span of L elements is (z^L, B) and only B is scanned or
// published — the slopes z^8, z^16 .. z^2048, z^(2048*64) come from the host as kernel arguments.
//
// THREE-PHASE (further down): chunk values / scan of the chunk values (recursively, down to one workgroup) / replay.  Five launches
// per call, every element read twice with 512-byte or 1-KiB strides between lanes; it needs 4-byte alignment only.
#define BX_PLAIN_MAD 1  // the signed multiply-adds of lazy_ext.hpp are left to the compiler here
#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "lazy_ext.hpp"

namespace bx {

constexpr int SC_T = 256, SC_I = 8, SC_TILE = SC_T * SC_I;
constexpr uint32_t SC_VALID = 0x80000000u;
constexpr uint32_t SC_HDR = 4;  // words before a sequence's slots: [0] ticket

__device__ __forceinline__ Fp4 sc_ld4(const uint32_t* p) {
    uint4 v = *reinterpret_cast<const uint4*>(p);
    return Fp4{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ uint4 sc_u4(const Fp4& a) { return make_uint4(a.c[0], a.c[1], a.c[2], a.c[3]); }
__device__ __forceinline__ void sc_st4(uint32_t* p, const Fp4& a) { *reinterpret_cast<uint4*>(p) = sc_u4(a); }
__device__ __forceinline__ void sc_publish(uint32_t* slot, const Fp4& v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) __hip_atomic_store(slot + k, v.c[k] | SC_VALID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool sc_try_read(const uint32_t* slot, Fp4& v) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = __hip_atomic_load(slot + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!((w[0] & w[1] & w[2] & w[3]) & SC_VALID)) return false;
#pragma unroll
    for (int k = 0; k < 4; ++k) v.c[k] = w[k] & ~SC_VALID;
    return true;
}
__device__ __forceinline__ Fp4 sc_shfl_up(const Fp4& v, int d) {
    return Fp4{{(uint32_t)__shfl_up((int)v.c[0], d), (uint32_t)__shfl_up((int)v.c[1], d), (uint32_t)__shfl_up((int)v.c[2], d),
                (uint32_t)__shfl_up((int)v.c[3], d)}};
}
__device__ __forceinline__ Fp4 sc_shfl_xor(const Fp4& v, int d) {
    return Fp4{{(uint32_t)__shfl_xor((int)v.c[0], d), (uint32_t)__shfl_xor((int)v.c[1], d), (uint32_t)__shfl_xor((int)v.c[2], d),
                (uint32_t)__shfl_xor((int)v.c[3], d)}};
}
// every thread of the grid clears its share of the other state buffer; then the workgroup draws its tile number
__device__ __forceinline__ uint32_t sc_begin(uint32_t* __restrict__ seq_state, uint32_t* __restrict__ clear, size_t clear_words, uint32_t* sh_tile) {
    const size_t nthreads = (size_t)gridDim.x * gridDim.y * blockDim.x;
    for (size_t i = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x; i < clear_words; i += nthreads) clear[i] = 0u;
    if (threadIdx.x == 0) *sh_tile = atomicAdd(seq_state, 1u);
    __syncthreads();
    return *sh_tile;
}

// ---- the two scan operators.  combine is the generic product, combine_lz the lazy one of the chains inside a tile (the same canonical
// words, so published values keep bit 31 free; the sum has one body for both, on purpose); pad is what an element past the end of a tile reads as; carry / apply are the last step,
// a lane's carry-in applied to its 8 running values: the product centres the carry once ----
struct ScanMul {
    using Carry = C4;
    static __device__ __forceinline__ Fp4 identity() { return f4_one(); }
    static __device__ __forceinline__ Fp4 combine(const Fp4& a, const Fp4& b) { return f4_mul(a, b); }
    static __device__ __forceinline__ Fp4 combine_lz(const Fp4& a, const Fp4& b) { return f4_mul_lz(a, b); }
    static __device__ __forceinline__ uint4 pad() { return make_uint4(MONT_ONE, 0, 0, 0); }
    static __device__ __forceinline__ Carry carry(const Fp4& e) { return f4_centre(e); }
    static __device__ __forceinline__ Fp4 apply(const Carry& e, const Fp4& x) { return f4_mul_cc(e, f4_centre(x)); }
};
struct ScanSum {
    using Carry = Fp4;
    static __device__ __forceinline__ Fp4 identity() { return f4_zero(); }
    static __device__ __forceinline__ Fp4 combine(const Fp4& a, const Fp4& b) { return f4_add(a, b); }
    static __device__ __forceinline__ Fp4 combine_lz(const Fp4& a, const Fp4& b) { return f4_add(a, b); }
    static __device__ __forceinline__ uint4 pad() { return make_uint4(0, 0, 0, 0); }
    static __device__ __forceinline__ Carry carry(const Fp4& e) { return e; }
    static __device__ __forceinline__ Fp4 apply(const Carry& e, const Fp4& x) { return f4_add(e, x); }
};

// ---- the pieces every tile kernel shares ----
// LDS layout of a tile: lane t's 8 elements at [9 t, 9 t + 8) (in 16-byte units): the pad makes the blocked accesses conflict-free
__device__ __forceinline__ uint32_t sc_slot(uint32_t u) { return (u >> 3) * 9u + (u & 7u); }
// Where element u of a tile lies in its sequence: ascending from `lo`, or (the division) descending from below `hi`.
struct TileUp {
    size_t lo;
    __device__ __forceinline__ size_t operator()(uint32_t u) const { return lo + u; }
};
struct TileDown {
    size_t hi;
    __device__ __forceinline__ size_t operator()(uint32_t u) const { return hi - 1 - u; }
};
// Coalesced load, transposed through LDS: element u of the tile is seq[at(u)], elements past `valid` read as `pad`; x[] returns the
// lane's 8 consecutive elements.  also(u) runs beside each element's load, so that whatever else a kernel stages per element (the
// LogUp multiplicities) is in flight together with the tile and behind the same barrier.
template <typename At, typename Also>
__device__ __forceinline__ void sc_tile_load(uint4* sh, const uint4* seq, At at, uint32_t valid, const uint4 pad, Fp4 (&x)[SC_I], Also also) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < SC_I; ++k) {
        const uint32_t u = (uint32_t)k * SC_T + tid;
        also(u);
        sh[sc_slot(u)] = u < valid ? seq[at(u)] : uint4(pad);  // a copy: between two lvalues the choice would be of addresses, one of them in scratch
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SC_I; ++k) {
        const uint4 w = sh[9 * tid + k];
        x[k] = Fp4{{w.x, w.y, w.z, w.w}};
    }
}
template <typename At>
__device__ __forceinline__ void sc_tile_load(uint4* sh, const uint4* seq, At at, uint32_t valid, const uint4 pad, Fp4 (&x)[SC_I]) {
    sc_tile_load(sh, seq, at, valid, pad, x, [](uint32_t) {});
}
// the way back: lane t has left its results at sh[9 t + k]
template <typename At>
__device__ __forceinline__ void sc_tile_store(const uint4* sh, uint4* seq, At at, uint32_t valid) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SC_I; ++k) {
        const uint32_t u = (uint32_t)k * SC_T + threadIdx.x;
        if (u < valid) seq[at(u)] = sh[sc_slot(u)];
    }
}
// The look-back of wave 0 (tile > 0): lane l inspects tile (base - l); tiles before the first one count as "inclusive, identity".
// Returns the carry entering `tile`.  W weighs what is read: W::lane a lane's value, W::window the combined window, W::next steps
// back one window — nothing for a plain operator, the known slopes for the division.
struct NoWeight {
    __device__ __forceinline__ Fp4 lane(const Fp4& v) const { return v; }
    __device__ __forceinline__ Fp4 window(const Fp4& p) const { return p; }
    __device__ __forceinline__ void next() {}
};
template <typename Op, typename W>
__device__ __forceinline__ Fp4 sc_look_back(const uint32_t* st, uint32_t tile, uint32_t lane, W w) {
    Fp4 carry = Op::identity();
    int base = (int)tile - 1;
    while (tile > 0) {
        const int id = base - (int)lane;
        Fp4 val = Op::identity();
        bool is_incl = true;
        if (id >= 0) {
            const uint32_t* slot = st + SC_HDR + 8 * (size_t)id;
            for (;;) {
                if (sc_try_read(slot + 4, val)) { is_incl = true; break; }
                if (sc_try_read(slot, val)) { is_incl = false; break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        const unsigned long long m = __ballot(is_incl);
        const uint32_t first = m ? (uint32_t)__ffsll((long long)m) - 1u : 64u;  // nearest tile whose inclusive value is known
        Fp4 part = lane <= first ? w.lane(val) : Op::identity();
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) part = Op::combine_lz(part, sc_shfl_xor(part, d));
        carry = Op::combine_lz(carry, w.window(part));
        if (first < 64u) break;
        w.next();
        base -= 64;
    }
    return carry;
}

struct DivSeq {
    Fp4 z;      // the point
    Fp4 zp[6];  // z^(8 * 2^k), k < 6: slopes of spans of 1, 2, .. 32 lanes
    Fp4 z512;   // slope of a wave (64 lanes x 8)
    Fp4 zL;     // slope of a tile
    Fp4 zLp[6]; // zL^(2^k), k < 6: a lane's look-back weight zL^lane is the product over the set bits of its number
    Fp4 zL64;   // slope of 64 tiles
    uint32_t poly, pad[3];  // which polynomial of the buffer this sequence divides
};
// base^lane from the table of base^(2^k): at most six lazy products instead of a square-and-multiply ladder of generic ones
__device__ __forceinline__ Fp4 sc_lane_pow(const Fp4 (&tab)[6], uint32_t lane) {
    Fp4 r = f4_one();
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const Fp4 t = f4_mul_lz(r, tab[k]);
        if (lane & (1u << k)) r = t;
    }
    return r;
}
struct DivArgs {
    DivSeq s[8];
};
// the division's look-back is a sum whose terms carry slopes: tile (base - l) weighs zL^l, the window `wbase`, 64 tiles zL64
struct DivWeight {
    const DivSeq& S;
    Fp4 lpow, wbase;
    __device__ __forceinline__ Fp4 lane(const Fp4& v) const { return f4_mul_lz(lpow, v); }
    __device__ __forceinline__ Fp4 window(const Fp4& p) const { return f4_mul(wbase, p); }
    __device__ __forceinline__ void next() { wbase = f4_mul(wbase, S.zL64); }
};

__global__ __launch_bounds__(SC_T) void div_lookback_kernel(uint32_t* __restrict__ polys, size_t size, DivArgs args, uint32_t* __restrict__ state,
                                                            uint32_t seq_stride, uint32_t tiles, uint32_t* __restrict__ clear, size_t clear_words,
                                                            uint32_t* __restrict__ rems) {
    __shared__ uint4 sh[SC_T * 9];
    __shared__ uint32_t wtot[4 * 4], carry_sh[4], agg_sh[4], sh_tile;
    const uint32_t q = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t* st = state + (size_t)q * seq_stride;
    const uint32_t tile = sc_begin(st, clear, clear_words, &sh_tile);
    const DivSeq& S = args.s[q];
    uint4* poly = reinterpret_cast<uint4*>(polys) + (size_t)S.poly * size;
    const size_t hi = size - (size_t)tile * SC_TILE;                    // positions [hi - valid, hi), top first: u = hi - 1 - pos
    const uint32_t valid = hi < (size_t)SC_TILE ? (uint32_t)hi : (uint32_t)SC_TILE;  // elements of this tile that exist
    Fp4 v[SC_I];
    sc_tile_load(sh, poly, TileDown{hi}, valid, make_uint4(0, 0, 0, 0), v);
    const uint32_t mine = valid > SC_I * tid ? (valid - SC_I * tid < (uint32_t)SC_I ? valid - SC_I * tid : (uint32_t)SC_I) : 0u;
    const C4 zc = f4_centre(S.z);
    Fp4 cur = f4_zero();
#pragma unroll
    for (int k = 0; k < SC_I; ++k)
        if ((uint32_t)k < mine) cur = f4_add(f4_mul_cc(zc, f4_centre(cur)), v[k]);
    // inclusive scan over the lanes of a wave: I_t = z^8 I_(t-1) + B_t, by doubling with the known slopes
    Fp4 I = cur;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const Fp4 prev = sc_shfl_up(I, 1 << k);
        if (lane >= (1u << k)) I = f4_add(I, f4_mul_lz(S.zp[k], prev));
    }
    if (lane == 63) sc_st4(wtot + 4 * wv, I);
    __syncthreads();
    Fp4 cw = f4_zero();  // carry entering this wave from the waves above it (tile carry still zero)
    for (uint32_t w = 0; w < wv; ++w) cw = f4_add(f4_mul_lz(S.z512, cw), sc_ld4(wtot + 4 * w));
    const Fp4 zlane = sc_lane_pow(S.zp, lane);  // z^(8 lane): what a carry entering the wave is multiplied by on its way to this lane
    Fp4 excl = sc_shfl_up(I, 1);
    if (lane == 0) excl = f4_zero();
    excl = f4_add(excl, f4_mul_lz(zlane, cw));
    if (tid == SC_T - 1) {
        const Fp4 agg = f4_add(I, f4_mul(S.z512, cw));  // the whole tile with zero carry-in
        sc_st4(agg_sh, agg);
        if (tile > 0) sc_publish(st + SC_HDR + 8 * (size_t)tile, agg);
    }
    __syncthreads();
    if (wv == 0) {
        const Fp4 carry = sc_look_back<ScanSum>(st, tile, lane, DivWeight{S, sc_lane_pow(S.zLp, lane), f4_one()});
        if (lane == 0) {
            const Fp4 incl = f4_add(f4_mul(S.zL, carry), sc_ld4(agg_sh));
            sc_publish(st + SC_HDR + 8 * (size_t)tile + 4, incl);
            sc_st4(carry_sh, carry);
        }
    }
    __syncthreads();
    // replay: the carry entering this lane, then its elements
    Fp4 zt = zlane;
    for (uint32_t w = 0; w < wv; ++w) zt = f4_mul_lz(zt, S.z512);
    cur = f4_add(excl, f4_mul_lz(zt, sc_ld4(carry_sh)));
#pragma unroll
    for (int k = 0; k < SC_I; ++k) {
        if (SC_I * tid + (uint32_t)k < valid) {  // k < mine, said again from `valid`: the eight masks of the first pass are not kept across the look-back
            sh[9 * tid + k] = sc_u4(cur);
            cur = f4_add(f4_mul_cc(zc, f4_centre(cur)), v[k]);
        }
    }
    // the lane that owns coefficient 0 leaves the division with the remainder in `cur`
    if (tile == tiles - 1 && mine > 0 && SC_I * tid + mine == valid) sc_st4(rems + 4 * (size_t)q, cur);
    sc_tile_store(sh, poly, TileDown{hi}, valid);
}

// ---- batch inversion: Montgomery's trick over the K elements a lane holds: running products, ONE inversion of the last of them, and
// a walk back that peels one element off per step — 3 (K - 1) products and one exponentiation instead of K exponentiations.  A zero
// element takes part as 1 and comes out as 0 (selects, no branches), so it does not poison its chunk; results are canonical, hence
// equal word for word to K separate inversions.
struct InvFp {
    using T = uint32_t;
    static __device__ __forceinline__ T one() { return MONT_ONE; }
    static __device__ __forceinline__ bool is_zero(T a) { return a == 0u; }
    static __device__ __forceinline__ T mul(T a, T b) { return fp_mul(a, b); }
    static __device__ __forceinline__ T inv(T a) { return fp_inv(a); }
    static __device__ __forceinline__ T pick(bool z, T a) { return z ? 0u : a; }
};
struct InvFp4 {
    using T = Fp4;
    static __device__ __forceinline__ T one() { return f4_one(); }
    static __device__ __forceinline__ bool is_zero(const T& a) { return f4_is_zero(a); }
    static __device__ __forceinline__ T mul(const T& a, const T& b) { return f4_mul_lz(a, b); }
    static __device__ __forceinline__ T inv(const T& a) { return f4_inv(a); }
    static __device__ __forceinline__ T pick(bool z, const T& a) { return Fp4{{z ? 0u : a.c[0], z ? 0u : a.c[1], z ? 0u : a.c[2], z ? 0u : a.c[3]}}; }
};
template <typename F, int K>
__device__ __forceinline__ void inv_chunk(typename F::T (&x)[K]) {
    using T = typename F::T;
    T pre[K];
    uint32_t zeros = 0u;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const bool z = F::is_zero(x[k]);
        zeros |= (z ? 1u : 0u) << k;
        if (z) x[k] = F::one();
        pre[k] = k ? F::mul(pre[k - 1], x[k]) : x[k];
    }
    T inv = F::inv(pre[K - 1]);  // of a product of non-zero elements: never zero
#pragma unroll
    for (int k = K - 1; k > 0; --k) {
        const T o = F::mul(inv, pre[k - 1]);
        inv = F::mul(inv, x[k]);
        x[k] = F::pick((zeros >> k) & 1u, o);
    }
    x[0] = F::pick(zeros & 1u, inv);
}

// The scan of `count` sequences of n elements back to back, forward: out[i] <- in[0] op .. op in[i] (prefix_products with ScanMul,
// prefix_sums with ScanSum).  What a tile does to its elements before it scans them is the pre-step:
//   PRE_LOGUP (sums only): the element that enters the sum is mults[i] * in[i]^-1, formed in the tile load — a lane's 8 elements are
//   one inversion chunk — so the fused call reads denoms and mults once and writes out once.
//   PRE_RATIO (products only): the element that enters the product is in[i] * den[i]^-1, where `mults` points at the AoS ext
//   denominators.  The tile of denominators goes through `sh` first and is inverted like a LogUp chunk; the tile of numerators then
//   takes the same 36 KiB (a second static tile would pass 64 KiB of static LDS), behind the barrier its write needs after the
//   first tile's reads.  Past the end both read as one.  Both arrays are read once, out is written once.
// in == out is allowed: a tile reads only itself, before it writes.  `mults` is never written and never overlaps out.
__device__ __forceinline__ uint32_t sc_mslot(uint32_t u) { return u + (u >> 5); }  // 8 words per lane, 32 banks: lanes 4 apart shift by one bank
enum ScanPre { PRE_NONE, PRE_LOGUP, PRE_RATIO };
template <typename Op, ScanPre PRE>
__global__ __launch_bounds__(SC_T) void scan_lookback_kernel(const uint32_t* in, uint32_t* out, const uint32_t* __restrict__ mults, size_t n,
                                                             uint32_t* __restrict__ state, uint32_t seq_stride, uint32_t* __restrict__ clear,
                                                             size_t clear_words) {
    __shared__ uint4 sh[SC_T * 9];
    constexpr bool LOGUP = PRE == PRE_LOGUP;
    __shared__ uint32_t shm[LOGUP ? SC_TILE + SC_TILE / 32 : 1];
    __shared__ uint32_t wtot[4 * 4], carry_sh[4], agg_sh[4], sh_tile;
    const uint32_t q = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t* st = state + (size_t)q * seq_stride;
    const uint32_t tile = sc_begin(st, clear, clear_words, &sh_tile);
    const size_t lo = (size_t)tile * SC_TILE;
    const uint4* src = reinterpret_cast<const uint4*>(in) + (size_t)q * n;
    uint4* dst = reinterpret_cast<uint4*>(out) + (size_t)q * n;
    const uint32_t valid = n - lo < (size_t)SC_TILE ? (uint32_t)(n - lo) : (uint32_t)SC_TILE;
    Fp4 pre[SC_I];  // this lane's elements, then their running values; elements past the end are identities: they change no running value
    Fp4 den[PRE == PRE_RATIO ? SC_I : 1];
    if constexpr (PRE == PRE_RATIO) {
        sc_tile_load(sh, reinterpret_cast<const uint4*>(mults) + (size_t)q * n, TileUp{lo}, valid, Op::pad(), den);
        inv_chunk<InvFp4, SC_I>(den);
        __syncthreads();  // every lane has read its denominators: the numerators may take the tile
    }
    sc_tile_load(sh, src, TileUp{lo}, valid, Op::pad(), pre, [=](uint32_t u) {
        if (LOGUP) shm[sc_mslot(u)] = u < valid ? mults[(size_t)q * n + lo + u] : 0u;
    });
    if (LOGUP) {
        inv_chunk<InvFp4, SC_I>(pre);
#pragma unroll
        for (int k = 0; k < SC_I; ++k) pre[k] = f4_scale(pre[k], shm[sc_mslot(SC_I * tid + (uint32_t)k)]);
    }
    if constexpr (PRE == PRE_RATIO) {
#pragma unroll
        for (int k = 0; k < SC_I; ++k) pre[k] = f4_mul_lz(pre[k], den[k]);
    }
#pragma unroll
    for (int k = 1; k < SC_I; ++k) pre[k] = Op::combine_lz(pre[k - 1], pre[k]);
    Fp4 I = pre[SC_I - 1];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const Fp4 prev = sc_shfl_up(I, 1 << k);
        if (lane >= (1u << k)) I = Op::combine_lz(I, prev);
    }
    if (lane == 63) sc_st4(wtot + 4 * wv, I);
    __syncthreads();
    Fp4 cw = Op::identity();
    for (uint32_t w = 0; w < wv; ++w) cw = Op::combine_lz(cw, sc_ld4(wtot + 4 * w));
    Fp4 excl = sc_shfl_up(I, 1);
    if (lane == 0) excl = Op::identity();
    excl = Op::combine_lz(excl, cw);
    if (tid == SC_T - 1) {
        const Fp4 agg = Op::combine(I, cw);
        sc_st4(agg_sh, agg);
        if (tile > 0) sc_publish(st + SC_HDR + 8 * (size_t)tile, agg);
    }
    __syncthreads();
    if (wv == 0) {
        const Fp4 carry = sc_look_back<Op>(st, tile, lane, NoWeight{});
        if (lane == 0) {
            sc_publish(st + SC_HDR + 8 * (size_t)tile + 4, Op::combine(carry, sc_ld4(agg_sh)));
            sc_st4(carry_sh, carry);
        }
    }
    __syncthreads();
    const typename Op::Carry e = Op::carry(Op::combine_lz(excl, sc_ld4(carry_sh)));
#pragma unroll
    for (int k = 0; k < SC_I; ++k) sh[9 * tid + k] = sc_u4(Op::apply(e, pre[k]));
    sc_tile_store(sh, dst, TileUp{lo}, valid);
}

// out[i] = in[i]^-1 (times mults[i] when BINV_SCALE) over n AoS ext elements; in == out is allowed.  A workgroup owns a tile of 2048
// elements, loaded coalesced and transposed through LDS like the scans, so that a lane inverts 8 consecutive elements.  Elements
// past the end are zeros: they cost a select and are never stored.
// BINV_RATIO: out[i] = in[i] * den[i]^-1, where `mults` points at the AoS ext denominators (never written, never overlapping out): the
// tile that is loaded and inverted is theirs, and a lane reads its own 8 numerators from `in` (in == out is allowed here too: every
// read of a tile comes before the barrier of its store).
enum BinvMode { BINV_PLAIN, BINV_SCALE, BINV_RATIO };
template <BinvMode MODE>
__global__ __launch_bounds__(SC_T) void binv_ext_kernel(const uint32_t* in, uint32_t* out, const uint32_t* __restrict__ mults, size_t n) {
    constexpr bool SCALE = MODE == BINV_SCALE;
    __shared__ uint4 sh[SC_T * 9];
    const uint32_t tid = threadIdx.x;
    const size_t lo = (size_t)blockIdx.x * SC_TILE;
    const uint32_t valid = n - lo < (size_t)SC_TILE ? (uint32_t)(n - lo) : (uint32_t)SC_TILE;
    Fp4 x[SC_I];
    sc_tile_load(sh, reinterpret_cast<const uint4*>(MODE == BINV_RATIO ? mults : in), TileUp{lo}, valid, make_uint4(0, 0, 0, 0), x);
    inv_chunk<InvFp4, SC_I>(x);
#pragma unroll
    for (int k = 0; k < SC_I; ++k) {
        if constexpr (MODE == BINV_RATIO) {  // 16-byte loads 128 bytes apart between lanes — the scan_lookback = 0 path only
            const uint32_t u = SC_I * tid + (uint32_t)k;
            if (u < valid) x[k] = f4_mul_lz(sc_ld4(in + 4 * (lo + u)), x[k]);
        }
        if (SCALE) {  // a lane reads its own 8 multiplicities: 4-byte loads 32 bytes apart, uncoalesced — this is the scan_lookback = 0 path only
            const uint32_t u = SC_I * tid + (uint32_t)k;
            x[k] = f4_scale(x[k], u < valid ? mults[lo + u] : 0u);
        }
        sh[9 * tid + k] = sc_u4(x[k]);
    }
    sc_tile_store(sh, reinterpret_cast<uint4*>(out), TileUp{lo}, valid);
}
// the same over base-field words, in place: a lane owns 8 consecutive words (two 16-byte accesses when the buffer is 16-byte aligned
// and the chunk is whole, single words otherwise)
constexpr int BI_K = 8;
__global__ __launch_bounds__(256) void binv_elem_kernel(uint32_t* __restrict__ io, size_t n, bool aligned16) {
    const size_t lo = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * BI_K;
    if (lo >= n) return;
    const bool whole = aligned16 && n - lo >= (size_t)BI_K;
    uint32_t x[BI_K];
    if (whole) {
        const uint4 a = *reinterpret_cast<const uint4*>(io + lo), b = *reinterpret_cast<const uint4*>(io + lo + 4);
        x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w, x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < BI_K; ++k) x[k] = lo + k < n ? io[lo + k] : 0u;
    }
    inv_chunk<InvFp, BI_K>(x);
    if (whole) {
        *reinterpret_cast<uint4*>(io + lo) = make_uint4(x[0], x[1], x[2], x[3]);
        *reinterpret_cast<uint4*>(io + lo + 4) = make_uint4(x[4], x[5], x[6], x[7]);
    } else {
#pragma unroll
        for (int k = 0; k < BI_K; ++k)
            if (lo + k < n) io[lo + k] = x[k];
    }
}

// ---- the three-phase forms ----
// The chunk walks below are chains of dependent Fp4 products; their loads are independent, so they are issued eight at a
// time (SCAN_B elements = 128 bytes per lane in flight) instead of one per product.
constexpr int SCAN_B = 8;

// poly_divide: q_{i-1} = p_i + z q_i (top down), in place; remainder = p_0 + z q_0.
// Three phases over chunks of DIV_L coefficients: (1) each chunk's carry-out assuming zero carry-in,
// (2) sequential composition of the chunk maps carry -> local + z^L * carry (one workgroup), (3) replay.
// The phases nest: the chunk values are themselves an array to be divided by (x - z^L) — "the carry entering chunk ch" is
// that division's quotient coefficient — so arrays longer than DIV_DIRECT recurse with chunks of DIV_L and the one-workgroup
// kernel only ever sees <= DIV_DIRECT entries (2^20 -> 2^15 -> 2^10: five launches).
constexpr int DIV_L = 32;
constexpr size_t DIV_DIRECT = 2048;
__global__ void div_local_kernel(const uint32_t* __restrict__ poly, size_t size, Fp4 z, uint32_t* __restrict__ local,
                                 size_t chunks) {
    size_t ch = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= chunks) return;
    size_t lo = ch * DIV_L, hi = lo + DIV_L < size ? lo + DIV_L : size;
    Fp4 cur = f4_zero();
    for (size_t top = hi; top > lo;) {
        const size_t nb = top - lo < (size_t)SCAN_B ? top - lo : (size_t)SCAN_B;
        Fp4 v[SCAN_B];
#pragma unroll
        for (int k = 0; k < SCAN_B; ++k)
            if ((size_t)k < nb) v[k] = sc_ld4(poly + 4 * (top - 1 - k));
#pragma unroll
        for (int k = 0; k < SCAN_B; ++k)
            if ((size_t)k < nb) cur = f4_add(f4_mul(z, cur), v[k]);
        top -= nb;
    }
    sc_st4(local + 4 * ch, cur);
}
// carry_in[ch] = value of `cur` entering chunk ch from above.  One workgroup: thread t owns a contiguous run of chunks
// (thread 0 the highest), reduces it to the affine map carry -> a*carry + b, the maps are composed across threads with a
// log-step (Hillis-Steele) scan in LDS, and each thread replays its run with the carry that enters it.
__global__ void div_scan_kernel(uint32_t* __restrict__ local_then_carry, size_t chunks, Fp4 zL, uint32_t* __restrict__ rem) {
    extern __shared__ uint32_t sh[];  // per thread: a (4 words) | b (4 words)
    const uint32_t nt = blockDim.x, tid = threadIdx.x;
    size_t per = (chunks + nt - 1) / nt;
    size_t hi = chunks > (size_t)tid * per ? chunks - (size_t)tid * per : 0;
    size_t lo = hi > per ? hi - per : 0;
    Fp4 a = f4_one(), b = f4_zero();
    for (size_t ch = hi; ch-- > lo;) {
        b = f4_add(f4_mul(zL, b), sc_ld4(local_then_carry + 4 * ch));
        a = f4_mul(a, zL);
    }
    // inclusive scan of F_t = f_t o f_(t-1) o ... o f_0 with (a2,b2) o (a1,b1) = (a2*a1, a2*b1 + b2)
    for (uint32_t d = 1; d < nt; d <<= 1) {
        sc_st4(sh + 8 * tid, a);
        sc_st4(sh + 8 * tid + 4, b);
        __syncthreads();
        if (tid >= d) {
            Fp4 pa = sc_ld4(sh + 8 * (tid - d)), pb = sc_ld4(sh + 8 * (tid - d) + 4);
            b = f4_add(f4_mul(a, pb), b);
            a = f4_mul(a, pa);
        }
        __syncthreads();
    }
    sc_st4(sh + 8 * tid + 4, b);
    __syncthreads();
    if (tid == nt - 1) sc_st4(rem, b);  // composition of every run applied to carry 0 = the remainder
    Fp4 carry = tid == 0 ? f4_zero() : sc_ld4(sh + 8 * (tid - 1) + 4);
    for (size_t ch = hi; ch-- > lo;) {
        Fp4 l = sc_ld4(local_then_carry + 4 * ch);
        sc_st4(local_then_carry + 4 * ch, carry);
        carry = f4_add(f4_mul(zL, carry), l);
    }
}
__global__ void div_apply_kernel(uint32_t* __restrict__ poly, size_t size, Fp4 z, const uint32_t* __restrict__ carry_in,
                                 size_t chunks) {
    size_t ch = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= chunks) return;
    size_t lo = ch * DIV_L, hi = lo + DIV_L < size ? lo + DIV_L : size;
    Fp4 cur = sc_ld4(carry_in + 4 * ch);
    for (size_t top = hi; top > lo;) {
        const size_t nb = top - lo < (size_t)SCAN_B ? top - lo : (size_t)SCAN_B;
        Fp4 v[SCAN_B];
#pragma unroll
        for (int k = 0; k < SCAN_B; ++k)
            if ((size_t)k < nb) v[k] = sc_ld4(poly + 4 * (top - 1 - k));
#pragma unroll
        for (int k = 0; k < SCAN_B; ++k)
            if ((size_t)k < nb) {
                sc_st4(poly + 4 * (top - 1 - k), cur);
                cur = f4_add(f4_mul(z, cur), v[k]);
            }
        top -= nb;
    }
}

// prefix_products / prefix_sums: the same three-phase shape over an operator, chunks of PP_L elements, one lane per chunk.
constexpr int PP_L = 64;
constexpr size_t PP_DIRECT = 2048;
// agg[ch] <- the chunk's aggregate.  blockIdx.y = sequence of a batch (each with its own n elements of io and `chunks` aggregates)
template <typename Op>
__global__ void tp_local_kernel(const uint32_t* __restrict__ io, size_t n, size_t seq_stride, uint32_t* __restrict__ agg, size_t chunks,
                                size_t agg_stride) {
    size_t ch = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= chunks) return;
    io += 4 * seq_stride * blockIdx.y;
    agg += 4 * agg_stride * blockIdx.y;
    size_t lo = ch * PP_L, hi = lo + PP_L < n ? lo + PP_L : n;
    Fp4 p = Op::identity();
    for (size_t b = lo; b < hi; b += SCAN_B) {
        const size_t nb = hi - b < (size_t)SCAN_B ? hi - b : (size_t)SCAN_B;
        Fp4 v[SCAN_B];
#pragma unroll
        for (int k = 0; k < SCAN_B; ++k)
            if ((size_t)k < nb) v[k] = sc_ld4(io + 4 * (b + k));
#pragma unroll
        for (int k = 0; k < SCAN_B; ++k)
            if ((size_t)k < nb) p = Op::combine(p, v[k]);
    }
    sc_st4(agg + 4 * ch, p);
}
// agg[ch] <- aggregate of all chunks before ch (exclusive scan), one workgroup per sequence, log-step scan across threads
template <typename Op>
__global__ void tp_scan_kernel(uint32_t* __restrict__ agg, size_t chunks, size_t agg_stride) {
    extern __shared__ uint32_t sh[];
    agg += 4 * agg_stride * blockIdx.x;
    const uint32_t nt = blockDim.x, tid = threadIdx.x;
    size_t per = (chunks + nt - 1) / nt;
    size_t lo = (size_t)tid * per < chunks ? (size_t)tid * per : chunks;
    size_t hi = lo + per < chunks ? lo + per : chunks;
    Fp4 incl = Op::identity();
    for (size_t ch = lo; ch < hi; ++ch) incl = Op::combine(incl, sc_ld4(agg + 4 * ch));
    for (uint32_t d = 1; d < nt; d <<= 1) {
        sc_st4(sh + 4 * tid, incl);
        __syncthreads();
        if (tid >= d) incl = Op::combine(incl, sc_ld4(sh + 4 * (tid - d)));
        __syncthreads();
    }
    sc_st4(sh + 4 * tid, incl);
    __syncthreads();
    Fp4 carry = tid == 0 ? Op::identity() : sc_ld4(sh + 4 * (tid - 1));
    for (size_t ch = lo; ch < hi; ++ch) {
        Fp4 a = sc_ld4(agg + 4 * ch);
        sc_st4(agg + 4 * ch, carry);
        carry = Op::combine(carry, a);
    }
}
// io[i] <- carry op io[lo] op .. op io[i - 1] (EXCL, the inner levels) or .. op io[i] (the caller's array)
template <typename Op, bool EXCL>
__global__ void tp_apply_kernel(uint32_t* __restrict__ io, size_t n, size_t seq_stride, const uint32_t* __restrict__ carry_in, size_t chunks,
                                size_t carry_stride) {
    size_t ch = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= chunks) return;
    io += 4 * seq_stride * blockIdx.y;
    carry_in += 4 * carry_stride * blockIdx.y;
    size_t lo = ch * PP_L, hi = lo + PP_L < n ? lo + PP_L : n;
    Fp4 p = sc_ld4(carry_in + 4 * ch);
    for (size_t b = lo; b < hi; b += SCAN_B) {
        const size_t nb = hi - b < (size_t)SCAN_B ? hi - b : (size_t)SCAN_B;
        Fp4 v[SCAN_B];
#pragma unroll
        for (int k = 0; k < SCAN_B; ++k)
            if ((size_t)k < nb) v[k] = sc_ld4(io + 4 * (b + k));
#pragma unroll
        for (int k = 0; k < SCAN_B; ++k)
            if ((size_t)k < nb) {
                if (EXCL) sc_st4(io + 4 * (b + k), p);
                p = Op::combine(p, v[k]);
                if (!EXCL) sc_st4(io + 4 * (b + k), p);
            }
    }
}

// two alternating state buffers; returns the one to use and what to clear in the other
const char* scan_state(bx_ctx* c, size_t words, uint32_t** use, uint32_t** clear, size_t* clear_words) {
    if (c->scan_cap < words) {
        BX_HIP(c, stream_wait(c));
        for (int b = 0; b < 2; ++b) {
            if (c->d_scan[b]) BX_HIP(c, hipFree(c->d_scan[b]));
            c->d_scan[b] = nullptr;
        }
        size_t cap = words < ((size_t)1 << 16) ? ((size_t)1 << 16) : words;
        for (int b = 0; b < 2; ++b) {
            BX_HIP(c, hipMalloc(&c->d_scan[b], cap * 4));
            BX_HIP(c, hipMemsetAsync(c->d_scan[b], 0, cap * 4, c->stream));
            c->scan_used[b] = 0;
        }
        c->scan_cap = cap;
    }
    const int b = c->scan_next;
    c->scan_next ^= 1;
    *use = c->d_scan[b];
    *clear = c->d_scan[b ^ 1];
    *clear_words = c->scan_used[b ^ 1];
    c->scan_used[b ^ 1] = 0;  // this launch clears it
    c->scan_used[b] = words;
    return nullptr;
}

static DivSeq div_seq(const uint32_t z[4]) {
    DivSeq s;
    s.z = Fp4{{z[0], z[1], z[2], z[3]}};
    Fp4 p = f4_pow(s.z, SC_I);
    for (int k = 0; k < 6; ++k) {
        s.zp[k] = p;
        p = f4_mul(p, p);
    }
    s.z512 = p;                               // z^(8 * 64)
    s.zL = f4_mul(f4_mul(p, p), f4_mul(p, p));  // z^2048
    p = s.zL;
    for (int k = 0; k < 6; ++k) {
        s.zLp[k] = p;
        p = f4_mul(p, p);
    }
    s.zL64 = p;
    return s;
}

// `count` polynomials of `size` AoS ext coefficients back to back, polynomial q divided in place by (x - zs[q]); rems[4q..] = remainder
static const char* poly_divide_lookback(bx_ctx* c, uint32_t* polys, size_t size, size_t count, const uint32_t* zs, uint32_t* rems, const uint32_t* which) {
    const size_t tiles = (size + SC_TILE - 1) / SC_TILE;
    const uint32_t seq_stride = SC_HDR + 8 * (uint32_t)tiles;
    for (size_t q0 = 0; q0 < count; q0 += 8) {
        const size_t nq = count - q0 < 8 ? count - q0 : 8;
        DivArgs args;
        for (size_t q = 0; q < nq; ++q) {
            args.s[q] = div_seq(zs + 4 * (q0 + q));
            args.s[q].poly = which ? which[q0 + q] : (uint32_t)(q0 + q);
        }
        uint32_t *use, *clear;
        size_t clear_words;
        BX_TRY(scan_state(c, (size_t)seq_stride * nq, &use, &clear, &clear_words));
        hipLaunchKernelGGL(div_lookback_kernel, dim3((unsigned)tiles, (unsigned)nq), dim3(SC_T), 0, c->stream, polys, size, args, use,
                           seq_stride, (uint32_t)tiles, clear, clear_words, rems + 4 * q0);
        BX_LAUNCH_CHECK(c);
    }
    return nullptr;
}
// the look-back scan of `count` sequences of n elements, `in` to `out` (the same buffer; denoms and mults to out for PRE_LOGUP; nums, with
// the ext denominators in `mults`, to out for PRE_RATIO)
template <typename Op, ScanPre PRE>
static const char* scan_lookback(bx_ctx* c, const uint32_t* in, uint32_t* out, const uint32_t* mults, size_t n, size_t count) {
    const size_t tiles = (n + SC_TILE - 1) / SC_TILE;
    const uint32_t seq_stride = SC_HDR + 8 * (uint32_t)tiles;
    uint32_t *use, *clear;
    size_t clear_words;
    BX_TRY(scan_state(c, (size_t)seq_stride * count, &use, &clear, &clear_words));
    hipLaunchKernelGGL((scan_lookback_kernel<Op, PRE>), dim3((unsigned)tiles, (unsigned)count), dim3(SC_T), 0, c->stream, in, out, mults, n, use,
                       seq_stride, clear, clear_words);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}

// in-place division of the AoS ext array `arr` (n entries) by (x - z); `scratch` has room for every level's chunk values
static const char* divide_rec(bx_ctx* c, uint32_t* arr, size_t n, Fp4 z, uint32_t* scratch, uint32_t* rem) {
    if (n <= DIV_DIRECT) {
        // one workgroup: thread t owns a run of entries; the "chunk" multiplier of the kernel is z itself here
        unsigned nt = n >= 1024 ? 1024 : 64;
        hipLaunchKernelGGL(div_scan_kernel, dim3(1), dim3(nt), nt * 32, c->stream, arr, n, z, rem);
        BX_LAUNCH_CHECK(c);
        return nullptr;
    }
    const size_t chunks = (n + DIV_L - 1) / DIV_L;
    hipLaunchKernelGGL(div_local_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t*)arr, n, z, scratch,
                       chunks);
    BX_LAUNCH_CHECK(c);
    BX_TRY(divide_rec(c, scratch, chunks, f4_pow(z, DIV_L), scratch + 4 * chunks, rem));  // chunk values -> carries entering the chunks
    hipLaunchKernelGGL(div_apply_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, c->stream, arr, n, z, (const uint32_t*)scratch,
                       chunks);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
static size_t scan_scratch_words(size_t n, size_t L, size_t direct, size_t count) {
    size_t words = 8;
    while (n > direct) {
        n = (n + L - 1) / L;
        words += 4 * n * count;
    }
    return words;
}
// The running Op, in place, over `count` sequences of n entries (sequence k at arr + 4 * k * stride): chunk aggregates -> exclusive scan
// of them (recursively, PP_L per level, one workgroup per sequence at the bottom) -> replay of every chunk with its carry.  EXCL: the
// exclusive scan, which the inner levels are; the caller's array is the inclusive one.
template <typename Op, bool EXCL>
static const char* three_phase_rec(bx_ctx* c, uint32_t* arr, size_t n, size_t stride, size_t count, uint32_t* scratch) {
    if (EXCL && n <= PP_DIRECT) {
        unsigned nt = n >= 1024 ? 1024 : 64;
        hipLaunchKernelGGL((tp_scan_kernel<Op>), dim3((unsigned)count), dim3(nt), nt * 16, c->stream, arr, n, stride);
        BX_LAUNCH_CHECK(c);
        return nullptr;
    }
    const size_t chunks = (n + PP_L - 1) / PP_L;
    hipLaunchKernelGGL((tp_local_kernel<Op>), dim3((unsigned)((chunks + 255) / 256), (unsigned)count), dim3(256), 0, c->stream, (const uint32_t*)arr, n,
                       stride, scratch, chunks, chunks);
    BX_LAUNCH_CHECK(c);
    BX_TRY((three_phase_rec<Op, true>(c, scratch, chunks, chunks, count, scratch + 4 * chunks * count)));
    hipLaunchKernelGGL((tp_apply_kernel<Op, EXCL>), dim3((unsigned)((chunks + 255) / 256), (unsigned)count), dim3(256), 0, c->stream, arr, n, stride,
                       (const uint32_t*)scratch, chunks, chunks);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
template <typename Op>
static const char* scan_three_phase(bx_ctx* c, uint32_t* io, size_t n, size_t count) {
    const size_t chunks = (n + PP_L - 1) / PP_L;
    BX_TRY(ensure_scratch(c, 4 * chunks * count + scan_scratch_words(chunks, PP_L, PP_DIRECT, count)));
    return three_phase_rec<Op, false>(c, io, n, n, count, c->d_scratch);
}

}  // namespace bx

using namespace bx;

extern "C" const char* bx_poly_divide(bx_ctx* c, bx_buf poly, const uint32_t z[4], bx_buf rem_out) try {
    if (!c) return "bx_poly_divide: null ctx";
    BX_REQUIRE(c, poly.len % 4 == 0 && rem_out.len >= 4, "poly_divide: poly must be AoS ext, remainder buffer >= 4 words");
    BX_REQUIRE(c, !bufs_overlap(bx_buf{rem_out.dptr, 4}, poly), "poly_divide: rem_out and poly overlap");
    BX_ENTER(c);
    size_t size = poly.len / 4;
    if (!size) return nullptr;
    OpScope op(c, "poly_divide", 8.0 * (double)poly.len);
    if (c->scan_lookback && ((uintptr_t)poly.dptr & 15u) == 0 && ((uintptr_t)rem_out.dptr & 15u) == 0)
        return poly_divide_lookback(c, (uint32_t*)poly.dptr, size, 1, z, (uint32_t*)rem_out.dptr, nullptr);
    BX_TRY(ensure_scratch(c, scan_scratch_words(size, DIV_L, DIV_DIRECT, 1)));
    return divide_rec(c, (uint32_t*)poly.dptr, size, Fp4{{z[0], z[1], z[2], z[3]}}, c->d_scratch, (uint32_t*)rem_out.dptr);
} BX_ABI_CATCH(c, "bx_poly_divide")
extern "C" const char* bx_poly_divide_batch(bx_ctx* c, bx_buf polys, size_t count, const uint32_t* zs, bx_buf rems_out) try {
    if (!c) return "bx_poly_divide_batch: null ctx";
    BX_REQUIRE(c, count >= 1 && count <= 65535 && polys.len % (4 * count) == 0, "poly_divide_batch: the buffer does not split into `count` AoS ext polynomials");
    BX_REQUIRE(c, zs != nullptr && rems_out.len >= 4 * count, "poly_divide_batch: one point and one remainder slot per polynomial");
    BX_REQUIRE(c, !bufs_overlap(bx_buf{rems_out.dptr, 4 * count}, polys), "poly_divide_batch: rems_out and polys overlap");
    BX_REQUIRE(c, ((uintptr_t)polys.dptr & 15u) == 0 && ((uintptr_t)rems_out.dptr & 15u) == 0, "poly_divide_batch: buffers must be 16-byte aligned");
    BX_ENTER(c);
    const size_t size = polys.len / 4 / count;
    if (!size) return nullptr;
    OpScope op(c, "poly_divide", 8.0 * (double)polys.len);
    return poly_divide_lookback(c, (uint32_t*)polys.dptr, size, count, zs, (uint32_t*)rems_out.dptr, nullptr);
} BX_ABI_CATCH(c, "bx_poly_divide_batch")
extern "C" const char* bx_poly_divide_batch_indexed(bx_ctx* c, bx_buf polys, size_t n_polys, size_t count, const uint32_t* which, const uint32_t* zs,
                                                    bx_buf rems_out) try {
    if (!c) return "bx_poly_divide_batch_indexed: null ctx";
    BX_REQUIRE(c, n_polys >= 1 && n_polys <= polys.len / 4 && polys.len % (4 * n_polys) == 0, "poly_divide_batch_indexed: the buffer does not split into n_polys AoS ext polynomials");
    BX_REQUIRE(c, count <= 65535 && which != nullptr && zs != nullptr && rems_out.len >= 4 * count, "poly_divide_batch_indexed: one index, one point and one remainder slot per division");
    BX_REQUIRE(c, !bufs_overlap(bx_buf{rems_out.dptr, 4 * count}, polys), "poly_divide_batch_indexed: rems_out and polys overlap");
    BX_REQUIRE(c, ((uintptr_t)polys.dptr & 15u) == 0 && ((uintptr_t)rems_out.dptr & 15u) == 0, "poly_divide_batch_indexed: buffers must be 16-byte aligned");
    for (size_t q = 0; q < count; ++q) BX_REQUIRE(c, which[q] < n_polys, "poly_divide_batch_indexed: polynomial index out of range");
    {
        std::vector<uint32_t> seen(which, which + count);
        std::sort(seen.begin(), seen.end());
        BX_REQUIRE(c, std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "poly_divide_batch_indexed: a polynomial may be divided once per call");
    }
    BX_ENTER(c);
    const size_t size = polys.len / 4 / n_polys;
    if (!size || !count) return nullptr;
    OpScope op(c, "poly_divide", 32.0 * (double)size * (double)count);
    return poly_divide_lookback(c, (uint32_t*)polys.dptr, size, count, zs, (uint32_t*)rems_out.dptr, which);
} BX_ABI_CATCH(c, "bx_poly_divide_batch_indexed")

extern "C" const char* bx_batch_prefix_products(bx_ctx* c, bx_buf io, size_t count) try {
    if (!c) return "bx_batch_prefix_products: null ctx";
    BX_REQUIRE(c, io.len % 4 == 0, "prefix_products: buffer must hold AoS ext elements");
    BX_REQUIRE(c, count >= 1 && (io.len / 4) % count == 0, "prefix_products: the buffer does not split into `count` equal sequences");
    BX_REQUIRE(c, count <= 65535, "prefix_products: too many sequences");
    BX_ENTER(c);
    size_t n = io.len / 4 / count;
    if (n < 2) return nullptr;
    OpScope op(c, "prefix_products", 8.0 * (double)io.len);
    if (c->scan_lookback && ((uintptr_t)io.dptr & 15u) == 0)
        return scan_lookback<ScanMul, PRE_NONE>(c, (const uint32_t*)io.dptr, (uint32_t*)io.dptr, nullptr, n, count);
    return scan_three_phase<ScanMul>(c, (uint32_t*)io.dptr, n, count);
} BX_ABI_CATCH(c, "bx_batch_prefix_products")
extern "C" const char* bx_prefix_products(bx_ctx* c, bx_buf io) try {
    if (!c) return "bx_prefix_products: null ctx";
    return bx_batch_prefix_products(c, io, 1);
} BX_ABI_CATCH(c, "bx_prefix_products")

// ---- LogUp helpers: batch inversion, prefix sums, and both in one pass ----
// out[i] = in[i]^-1 (* mults[i]) over n ext elements, one launch
static const char* launch_invert_ext(bx_ctx* c, const uint32_t* in, uint32_t* out, const uint32_t* mults, size_t n) {
    const unsigned tiles = (unsigned)((n + SC_TILE - 1) / SC_TILE);
    if (mults)
        hipLaunchKernelGGL(binv_ext_kernel<BINV_SCALE>, dim3(tiles), dim3(SC_T), 0, c->stream, in, out, mults, n);
    else
        hipLaunchKernelGGL(binv_ext_kernel<BINV_PLAIN>, dim3(tiles), dim3(SC_T), 0, c->stream, in, out, mults, n);
    BX_LAUNCH_CHECK(c);
    return nullptr;
}
constexpr size_t SC_MAX_ELEMS = (size_t)SC_TILE << 28;  // tiles of one launch fit a grid dimension, and 8 state words per tile a 32-bit stride

extern "C" const char* bx_batch_invert_ext(bx_ctx* c, bx_buf io) try {
    if (!c) return "bx_batch_invert_ext: null ctx";
    BX_REQUIRE(c, io.len % 4 == 0, "batch_invert_ext: buffer must hold AoS ext elements");
    BX_REQUIRE(c, io.len / 4 <= SC_MAX_ELEMS, "batch_invert_ext: too many elements");
    BX_REQUIRE(c, ((uintptr_t)io.dptr & 15u) == 0, "batch_invert_ext: buffers must be 16-byte aligned");
    BX_ENTER(c);
    if (!io.len) return nullptr;
    OpScope op(c, "batch_invert_ext", 8.0 * (double)io.len);
    return launch_invert_ext(c, (const uint32_t*)io.dptr, (uint32_t*)io.dptr, nullptr, io.len / 4);
} BX_ABI_CATCH(c, "bx_batch_invert_ext")
extern "C" const char* bx_batch_invert_elem(bx_ctx* c, bx_buf io) try {
    if (!c) return "bx_batch_invert_elem: null ctx";
    BX_REQUIRE(c, io.len <= SC_MAX_ELEMS, "batch_invert_elem: too many elements");
    BX_REQUIRE(c, ((uintptr_t)io.dptr & 3u) == 0, "batch_invert_elem: buffer must be word aligned");
    BX_ENTER(c);
    if (!io.len) return nullptr;
    OpScope op(c, "batch_invert_elem", 8.0 * (double)io.len);
    const size_t lanes = (io.len + BI_K - 1) / BI_K;
    hipLaunchKernelGGL(binv_elem_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, c->stream, (uint32_t*)io.dptr, io.len,
                       ((uintptr_t)io.dptr & 15u) == 0);
    BX_LAUNCH_CHECK(c);
    return nullptr;
} BX_ABI_CATCH(c, "bx_batch_invert_elem")
extern "C" const char* bx_batch_prefix_sums(bx_ctx* c, bx_buf io, size_t count) try {
    if (!c) return "bx_batch_prefix_sums: null ctx";
    BX_REQUIRE(c, io.len % 4 == 0, "prefix_sums: buffer must hold AoS ext elements");
    BX_REQUIRE(c, count >= 1 && count <= 65535, "prefix_sums: the number of sequences must be in [1, 65535]");
    BX_REQUIRE(c, (io.len / 4) % count == 0, "prefix_sums: the buffer does not split into `count` equal sequences");
    BX_REQUIRE(c, io.len / 4 / count <= SC_MAX_ELEMS, "prefix_sums: sequences too long");
    BX_REQUIRE(c, ((uintptr_t)io.dptr & 15u) == 0, "prefix_sums: buffers must be 16-byte aligned");
    BX_ENTER(c);
    const size_t n = io.len / 4 / count;
    if (n < 2) return nullptr;
    OpScope op(c, "prefix_sums", 8.0 * (double)io.len);
    if (c->scan_lookback) return scan_lookback<ScanSum, PRE_NONE>(c, (const uint32_t*)io.dptr, (uint32_t*)io.dptr, nullptr, n, count);
    return scan_three_phase<ScanSum>(c, (uint32_t*)io.dptr, n, count);
} BX_ABI_CATCH(c, "bx_batch_prefix_sums")
extern "C" const char* bx_prefix_sums(bx_ctx* c, bx_buf io) try {
    if (!c) return "bx_prefix_sums: null ctx";
    return bx_batch_prefix_sums(c, io, 1);
} BX_ABI_CATCH(c, "bx_prefix_sums")
extern "C" const char* bx_logup_accumulate(bx_ctx* c, bx_buf out, bx_buf denoms, bx_buf mults, size_t count) try {
    if (!c) return "bx_logup_accumulate: null ctx";
    BX_REQUIRE(c, out.len % 4 == 0 && denoms.len == out.len, "logup_accumulate: out and denoms must hold the same number of AoS ext elements");
    BX_REQUIRE(c, count >= 1 && count <= 65535, "logup_accumulate: the number of sequences must be in [1, 65535]");
    BX_REQUIRE(c, (out.len / 4) % count == 0, "logup_accumulate: the buffers do not split into `count` equal sequences");
    const size_t n = out.len / 4 / count;
    BX_REQUIRE(c, out.len / 4 <= SC_MAX_ELEMS, "logup_accumulate: too many elements");  // bounds n, and the one-launch inversion over all sequences
    BX_REQUIRE(c, mul_le(count, n, mults.len), "logup_accumulate: one multiplicity per denominator");
    BX_REQUIRE(c, bufs_same(out, denoms) || !bufs_overlap(out, denoms), "logup_accumulate: out and denoms overlap");
    BX_REQUIRE(c, !bufs_overlap(out, bx_buf{mults.dptr, count * n}), "logup_accumulate: out and mults overlap");
    BX_REQUIRE(c, ((uintptr_t)out.dptr & 15u) == 0 && ((uintptr_t)denoms.dptr & 15u) == 0 && ((uintptr_t)mults.dptr & 3u) == 0,
               "logup_accumulate: ext buffers must be 16-byte aligned");
    BX_ENTER(c);
    if (!n) return nullptr;
    OpScope op(c, "logup_accumulate", 8.0 * (double)out.len + 4.0 * (double)(count * n));
    if (c->scan_lookback)
        return scan_lookback<ScanSum, PRE_LOGUP>(c, (const uint32_t*)denoms.dptr, (uint32_t*)out.dptr, (const uint32_t*)mults.dptr, n, count);
    // the three-phase form: invert and scale into out, then the three-phase running sums over out
    BX_TRY(launch_invert_ext(c, (const uint32_t*)denoms.dptr, (uint32_t*)out.dptr, (const uint32_t*)mults.dptr, n * count));
    if (n < 2) return nullptr;
    return scan_three_phase<ScanSum>(c, (uint32_t*)out.dptr, n, count);
} BX_ABI_CATCH(c, "bx_logup_accumulate")
extern "C" const char* bx_batch_ratio_products(bx_ctx* c, bx_buf out, bx_buf nums, bx_buf denoms, size_t count) try {
    if (!c) return "bx_batch_ratio_products: null ctx";
    BX_REQUIRE(c, out.len % 4 == 0 && nums.len == out.len && denoms.len == out.len,
               "bx_batch_ratio_products: out, nums and denoms must hold the same number of AoS ext elements");
    BX_REQUIRE(c, count >= 1 && count <= 65535, "bx_batch_ratio_products: the number of sequences must be in [1, 65535]");
    BX_REQUIRE(c, (out.len / 4) % count == 0, "bx_batch_ratio_products: the buffers do not split into `count` equal sequences");
    const size_t n = out.len / 4 / count;
    BX_REQUIRE(c, out.len / 4 <= SC_MAX_ELEMS, "bx_batch_ratio_products: too many elements");  // bounds n, and the one-launch inversion over all sequences
    BX_REQUIRE(c, bufs_same(out, nums) || !bufs_overlap(out, nums), "bx_batch_ratio_products: out and nums overlap");
    BX_REQUIRE(c, !bufs_overlap(out, denoms), "bx_batch_ratio_products: out and denoms overlap");
    BX_REQUIRE(c, ((uintptr_t)out.dptr & 15u) == 0 && ((uintptr_t)nums.dptr & 15u) == 0 && ((uintptr_t)denoms.dptr & 15u) == 0,
               "bx_batch_ratio_products: buffers must be 16-byte aligned");
    BX_ENTER(c);
    if (!n) return nullptr;
    OpScope op(c, "ratio_products", 12.0 * (double)out.len);
    // the ext denominators travel where the LogUp multiplicities do: read-only, and never overlapping out
    if (c->scan_lookback)
        return scan_lookback<ScanMul, PRE_RATIO>(c, (const uint32_t*)nums.dptr, (uint32_t*)out.dptr, (const uint32_t*)denoms.dptr, n, count);
    // the three-phase form: nums * denoms^-1 into out, then the three-phase running products over out
    hipLaunchKernelGGL(binv_ext_kernel<BINV_RATIO>, dim3((unsigned)((n * count + SC_TILE - 1) / SC_TILE)), dim3(SC_T), 0, c->stream, (const uint32_t*)nums.dptr,
                       (uint32_t*)out.dptr, (const uint32_t*)denoms.dptr, n * count);
    BX_LAUNCH_CHECK(c);
    if (n < 2) return nullptr;
    return scan_three_phase<ScanMul>(c, (uint32_t*)out.dptr, n, count);
} BX_ABI_CATCH(c, "bx_batch_ratio_products")
