// circuit_common.hpp — the frame the built-in circuits share (circuit.hip, lookup.hip): a circuit's own file holds its kernels
// and its bx_circuit_ops entries; what every such table needs around them lives here, once.
//   host    launch grids and seed derivations, the segment header, the noise seed of the next witgen, the mix-power table and the
//           vanishing-polynomial inverses of eval_check, the store of the accumulate step's ext runs into the accum group
//   device  the ends of an eval_check kernel: a mix power from the table, the mixing of a base-valued and of an ext-valued constraint, an
//           ext column at a point and one row back, the closing division
// The device inlines sit on lazy_ext.hpp and therefore in the same inline namespace as circuit_dev.hpp: a circuit's translation
// unit defines BX_PLAIN_MAD before it includes either.
#pragma once
#include "circuit.hpp"
#include "ctx.hpp"
#include "lazy_ext.hpp"
#include "../../include/bx_circuit.h"

namespace bx {

// blocks of a grid-stride launch over n elements
inline unsigned grid_for(size_t n, unsigned bs = 256, size_t cap = 1 << 16) {
    size_t b = (n + bs - 1) / bs;
    return (unsigned)(b > cap ? cap : (b ? b : 1));
}

// ---- seeds (bx_prover.h, "seeds"): the generators a witness is drawn from, as functions of the segment's seed ----
constexpr uint64_t GOLDEN64 = 0x9E3779B97F4A7C15ull;
// of the data group's cells, from the segment's seed (active rows) or from the noise seed (ZK rows)
inline uint64_t data_seed(uint64_t seed) { return seed + GOLDEN64 * 2; }
// of the accum group's filler columns: drawn after the accumulators' mix, so that they depend on it
inline uint64_t filler_seed(uint64_t seed, const uint32_t mix[4]) { return (seed + GOLDEN64 * 3) ^ (((uint64_t)mix[0] << 32) | mix[1]); }

// bx_circuit_ops::set_noise_seed: the generator of the ZK rows of the NEXT witgen, accepted or refused
struct NoiseSeed {
    uint64_t given = 0;
    bool armed = false;
    void set(uint64_t noise_seed) {
        given = noise_seed;
        armed = true;
    }
    // for this witgen: the seed given, else a function of the segment's seed; a given seed is used up either way
    uint64_t take(uint64_t seed) {
        const uint64_t noise = armed ? given : splitmix64(seed ^ 0x5A4B4E4F49534521ull);
        armed = false;
        return noise;
    }
};

// The header of a segment's bytes ("BXSYNSEG" | index | po2 | seed | payload): its seed, or why this prover cannot prove it.
const char* segment_header(bx_ctx* c, const uint8_t* segment, size_t segment_len, uint32_t po2, uint64_t* seed);

// What every eval_check needs: the table of n mix powers (canonical, then centred — the weights of LazyExtAcc: 8n words), and the
// four values 1 / ((3x)^N - 1) takes on the domain x = w_4N^row, indexed by row mod 4.
const char* mix_power_table(bx_ctx* c, bx_buf mixpows, const uint32_t poly_mix[4], uint32_t n);
void vanishing_inverses(uint32_t po2, uint32_t zinv[4]);

// The end of an accumulate step: ext sequence s of `run` (n_ext AoS runs of 2^po2 elements), component k -> accum column 4s + k;
// columns [4 n_ext, wa) are filler drawn from `seed`.  The caller has checked `accum` (wa columns of 2^po2 words) and owns `run`.
const char* store_ext_columns(bx_ctx* c, bx_buf accum, bx_buf run, uint32_t po2, uint32_t n_ext, uint32_t wa, uint64_t seed);

// what an eval_check kernel is told about its point set and statement
struct EvalPoint {
    uint32_t zinv[4];  // 1 / (3^N w_4^m - 1), m = row mod 4
    uint32_t g[2];     // the statement's public words
};

inline namespace BX_MAD_FLAVOUR {

// mix power k of a table (wave-uniform: one 16-byte scalar load)
__device__ __forceinline__ Fp4 mix_power(const uint32_t* __restrict__ mixpows, size_t k) {
    const uint4 m = *reinterpret_cast<const uint4*>(mixpows + 4 * k);
    return Fp4{{m.x, m.y, m.z, m.w}};
}
// acc += poly_mix^k * x for a base-valued constraint x: the weight comes from the centred half of the table
__device__ __forceinline__ void mix_add(LazyExtAcc& acc, const uint32_t* __restrict__ mixpows_c, size_t k, uint32_t x) {
    const Fp4 m = mix_power(mixpows_c, k);
    const i32 w[4] = {(i32)m.c[0], (i32)m.c[1], (i32)m.c[2], (i32)m.c[3]};
    acc.add(w, x);
}
// four centred words of a table (a mix power from the centred half, a challenge): wave-uniform, one 16-byte scalar load; the centring of
// a canonical table is scalar work
__device__ __forceinline__ void uniform_centred(const uint32_t* __restrict__ table, size_t k, bool canonical, i32 w[4]) {
    const Fp4 m = mix_power(table, k);
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = canonical ? fp_centre(m.c[q]) : (i32)m.c[q];
}
// acc += poly_mix^k * v for an ext-valued constraint v (|v[q]| <= P: lazy_ext.hpp), the weight from the centred half of the table
__device__ __forceinline__ void mix_add(WeightedExtAcc& acc, const uint32_t* __restrict__ mixpows_c, size_t k, const i32 v[4]) {
    i32 w[4];
    uniform_centred(mixpows_c, k, false, w);
    acc.add(w, v);
}
// ext column s of the accum group's evaluations (planes 4s .. 4s+3) at domain point i and one row back at ib, plane by plane: the two
// loads of a plane share their address arithmetic
__device__ __forceinline__ void ext_column_at(const uint32_t* __restrict__ eacc, uint32_t s, uint32_t dom, uint32_t i, uint32_t ib, Fp4& cur, Fp4& back) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cur.c[k] = eacc[(size_t)(4 * s + k) * dom + i];
        back.c[k] = eacc[(size_t)(4 * s + k) * dom + ib];
    }
}
// check(x) = tot / ((3x)^N - 1) into the four check planes
__device__ __forceinline__ void store_check(uint32_t* __restrict__ check, const Fp4& tot, const EvalPoint& pt, uint32_t dom, uint32_t i) {
    const Fp4 q = f4_scale(tot, pt.zinv[i & 3u]);
#pragma unroll
    for (int k = 0; k < 4; ++k) check[(size_t)k * dom + i] = q.c[k];
}

}  // inline namespace BX_MAD_FLAVOUR

}  // namespace bx
