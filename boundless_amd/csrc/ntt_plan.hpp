// ntt_plan.hpp — which kernels a batched NTT launches, decided on the host before the first launch (DESIGN.md §4 "The plan").
//
// Host-only and pure: no HIP header, no context, no pointer.  ntt_plan() maps (tunables, direction, size, expand / skip bits, columns
// of one launch, alignment, whether a post-factor is wanted) to the split 2^m = 2^m_hi * 2^m_lo and, for the contiguous pass A and the
// strided pass B, the kernel family, its compiled geometry and the launch shape — or to the error string of a shape that is refused.
// ntt.hip executes plans and decides nothing; tests/ntt_plan_check.cpp replays the launches recorded on the GPU
// (tests/golden/ntt_launches.json) and walks every tunable value in range through the same function without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bx {

constexpr int TW_LOG = 13;  // stage-twiddle tables cover sub-transform sizes up to 2^13

// bx_set_tunable("ntt_<member>") — names, ranges and tests in DESIGN.md §9
struct NttTunables {
    long block_log = 12;   // log2 of the contiguous-pass sub-transform, both families (13 when the size needs it)
    long tile_log = 14;    // v1 kernels: log2 of the strided-pass LDS tile (elements)
    long fast = 1;         // 1 = register-radix-16 passes (ntt_r16.hpp), 0 = one-stage-per-barrier v1 kernels
    long tile_a_log = 12;  // log2 elements per pass-A workgroup (radix-16)
    long tile_b_log = 13;  // log2 elements per pass-B workgroup (radix-16)
    long cols_per_wg = 8;  // forward pass A (2^12 tiles): columns sharing one load of the tile's twist + twiddles
    long group_cols = 0;   // forward transform: columns per pass-A + pass-B group (0 = all columns per pass)
    long tile_b_wide = 1;  // grow the pass-B tile (up to 2^14) so that rows are at least 16 words wide
};

// The compiled geometries of ntt_r16_kernel<INV, PASS_A, SKIP, LR, LT, MAXT>.  A pass takes the FIRST row of its kind whose
// condition holds: lr == LR and lt == LT for a specialised row; LR = 0 is the generic kernel (run-time lr / lt), whose 1024-thread
// row holds for tiles above 2^13 elements and whose 512-thread rows always hold.  The hot shapes (BASELINE sizes 2^20 / 2^22 and the
// po2 21 .. 24 segments at default tunables) get a specialisation: strided passes of 2^10 .. 2^13 rows on the 2^14-element tile
// (64-byte rows at 2^10), contiguous passes of 2^12 and 2^13.  A pass A with lr = 13 always has lrows = 13 (ntt_tile_a_log <= 13).
struct NttGeom {
    bool pass_a;
    int lr, lt, maxt;
};
constexpr NttGeom NTT_GEOMS[] = {
    {true, 12, 0, 512},  {false, 10, 3, 512},  {false, 10, 4, 1024}, {false, 11, 3, 1024}, {false, 12, 2, 1024}, {false, 13, 1, 1024},
    {true, 13, 0, 512},  {false, 0, 0, 1024},  {false, 8, 5, 512},   {true, 0, 0, 512},    {false, 0, 0, 512},
};
constexpr int NTT_GEOM_COUNT = (int)(sizeof NTT_GEOMS / sizeof NTT_GEOMS[0]);

enum NttFamily {
    NTT_ABSENT = 0,   // no such pass (a single-pass transform has no pass B)
    NTT_R16_GENERIC,  // ntt_r16_kernel, a row with LR = 0
    NTT_R16_GEOM,     // ntt_r16_kernel, a specialised row
    NTT_MULTI_A,      // ntt_passA_fwd12_multi_kernel: forward 2^12 pass A, several columns per workgroup
    NTT_V1,           // ntt_block_kernel (A) / ntt_strided_kernel (B)
};

struct NttPass {
    NttFamily family = NTT_ABSENT;
    int geom = -1;                  // row of NTT_GEOMS (radix-16 families)
    int lr = 0, lrows = 0, lt = 0;  // sub-transform 2^lr; tile of 2^lrows rows, 2^lt adjacent positions wide
    int row_shift = 0;              // log2 of the distance between consecutive rows (0 for pass A, m_hi for pass B)
    uint32_t tiles = 0;             // per column (v1 pass A: blocks per column)
    uint32_t threads = 0;           // per workgroup
    uint32_t cpw = 1;               // columns per workgroup (multi-column pass A)
    uint32_t grid_x = 0, grid_y = 1;
    size_t lds = 0;                 // dynamic LDS bytes
    bool r16() const { return family == NTT_R16_GENERIC || family == NTT_R16_GEOM || family == NTT_MULTI_A; }
};

struct NttPlan {
    const char* error = nullptr;  // set: the shape is refused and nothing else below is meaningful
    size_t count = 0;             // columns of one launch: the grids below are for this many
    int m_hi = 0, m_lo = 0;
    bool twist = false;  // two passes: the inter-pass twist table of (m, m_hi, direction) is needed
    NttPass a, b;
    bool post_on_a = false;  // inverse: the post-factor rides on pass A's final store (otherwise the caller applies it afterwards)
};

inline int ntt_geom_row(bool pass_a, int lr, int lrows, int lt) {
    for (int i = 0; i < NTT_GEOM_COUNT; ++i) {
        const NttGeom& g = NTT_GEOMS[i];
        if (g.pass_a != pass_a) continue;
        if (g.lr ? (lr == g.lr && lt == g.lt) : (g.maxt == 512 || lrows + lt > 13)) return i;
    }
    return -1;  // not reached: both kinds end in a row that always holds
}

// shape of a radix-16 launch of one tile per workgroup; nullptr or the reason it cannot be launched
inline const char* ntt_r16_shape(NttPass& p, bool pass_a, size_t count) {
    p.geom = ntt_geom_row(pass_a, p.lr, p.lrows, p.lt);
    p.family = NTT_GEOMS[p.geom].lr ? NTT_R16_GEOM : NTT_R16_GENERIC;
    const uint32_t tile_elems = 1u << (p.lrows + p.lt);
    p.lds = ((size_t)tile_elems + (tile_elems >> 4)) * 4;
    p.threads = tile_elems / 16;
    if (!((size_t)p.tiles * count < ((size_t)1 << 31))) return "ntt: too many workgroups in one launch";
    if (p.threads > (uint32_t)NTT_GEOMS[p.geom].maxt) return "ntt: tile larger than the kernel's launch bound";
    p.grid_x = p.tiles * (uint32_t)count;
    return nullptr;
}

// Plan of one transform of `count` columns of 2^m words (m >= 1, count >= 1).  Forward: `expand_bits` = load shift
// (out[i] = in[i >> bits]), `skip_bits` = leading stages skipped; the inverse takes 0 for both.  `aligned16`: in and out both start
// on a 16-byte boundary.  `want_post`: the caller has a per-position factor for the inverse's final store (the fused zk_shift).
inline NttPlan ntt_plan(const NttTunables& t, bool inverse, int m, int expand_bits, int skip_bits, size_t count, bool aligned16,
                        bool want_post) {
    NttPlan p;
    p.count = count;
    // ---- the split, for both families
    int blk = (int)t.block_log;
    if (blk > TW_LOG) blk = TW_LOG;
    // sizes beyond 2^24 (segments of po2 23 / 24): a taller contiguous pass keeps the strided pass at <= 2^12 rows where it can,
    // i.e. its LDS tile (<= 2^14 elements) at least four positions wide (measured: po2 23 proof 0.44 -> 0.38 s)
    if (m - blk > 12 && blk < TW_LOG) blk = m - 12 < TW_LOG ? m - 12 : TW_LOG;
    if (m <= blk) {
        p.m_hi = m;
        p.m_lo = 0;
    } else {
        p.m_hi = blk;
        p.m_lo = m - blk;
        if (p.m_lo > TW_LOG) {  // > 2^26: not reachable for BabyBear segment sizes
            p.m_lo = TW_LOG;
            p.m_hi = m - TW_LOG;
        }
    }
    const int m_hi = p.m_hi, m_lo = p.m_lo;
    if (m_hi > TW_LOG || m_lo > TW_LOG) return p.error = "ntt: size too large", p;
    if (!inverse && (expand_bits > m_hi || skip_bits > m_hi)) return p.error = "ntt: expand_bits larger than the block pass", p;
    p.twist = m_lo != 0;

    // ---- pass A: 2^m_lo contiguous blocks of 2^m_hi per column
    NttPass& a = p.a;
    a.lr = m_hi;
    int lrows = (int)t.tile_a_log;
    if (lrows < m_hi) lrows = m_hi;
    if (lrows > m) lrows = m;
    // radix-16: the tile must fill at least one wave (16 elements per lane) and every access is 16 bytes wide
    if (t.fast && lrows >= 10 && m_hi >= 1 && aligned16 && (((size_t)1 << m) >> expand_bits) % 4 == 0 &&
        (skip_bits == 0 || (skip_bits == 2 && !inverse))) {
        a.lrows = lrows;
        a.tiles = 1u << (m - lrows);
        if (!inverse && a.lr == 12 && a.lrows == 12 && t.cols_per_wg > 1 && count > 1 && (expand_bits == 0 || expand_bits == 2)) {
            a.family = NTT_MULTI_A;
            a.cpw = (uint32_t)t.cols_per_wg;
            a.threads = 256;
            a.lds = ((size_t)4096 + 256) * 4 * 2;  // two tiles, alternating by column
            a.grid_x = a.tiles * (uint32_t)((count + a.cpw - 1) / a.cpw);
        } else if ((p.error = ntt_r16_shape(a, true, count))) {
            return p;
        }
        // the final store of the inverse pass A applies the post-factor only in its 16-words-per-thread form (the last step is K = 4
        // at s0 = 0 whenever m_hi >= 4)
        p.post_on_a = inverse && want_post && m_hi >= 4;
    } else {  // v1: one workgroup per (block, column), LDS = data[R] + stage table[R]
        a.family = NTT_V1;
        a.lrows = m_hi;
        const uint32_t R = 1u << m_hi;
        a.tiles = 1u << m_lo;
        a.threads = R / 2 < 64 ? 64 : (R / 2 > 256 ? 256 : R / 2);
        a.lds = (size_t)R * 8;
        a.grid_x = a.tiles;
        a.grid_y = (uint32_t)count;
    }
    if (!m_lo) return p;

    // ---- pass B: 2^m_lo-point transforms across the blocks, 2^lt adjacent positions per workgroup
    NttPass& b = p.b;
    b.lr = b.lrows = m_lo;
    b.row_shift = m_hi;
    int tile = (int)t.tile_b_log;
    // keep every row access at least 64 bytes wide: tall passes (>= 2^10 rows) take the 2^14-element tile (1024 threads);
    // measured on the 2^22 LDE: -6 % time and 1.5x fewer HBM write bytes than 32-byte rows
    // ... and the tallest ones (2^11 .. 2^13 rows) the same 2^14-element tile, as wide as it still allows (po2 24 proof 1.22 -> 0.86 s)
    if (t.tile_b_wide && m_lo + 4 > tile) tile = m_lo + 4 <= 14 ? m_lo + 4 : 14;
    if (tile < m_lo) tile = m_lo;
    int lt = tile - m_lo;
    if (lt > m_hi) lt = m_hi;
    if (t.fast && m_lo + lt >= 10 && m_lo + lt <= 14) {
        // radix-16 pass B addresses a column through a buffer descriptor with 32-bit byte offsets and a 32-bit num_records
        // (ntt_r16.hpp glb_get / glb_put): a column must stay below 4 GiB, or loads past the wrap would return 0 and stores be dropped
        if ((((size_t)1 << m) * 4) >> 32 != 0) return p.error = "ntt: a column of 2^30 words or more does not fit pass B's 32-bit buffer offsets", p;
        b.lt = lt;
        b.tiles = 1u << (m_hi - lt);
        if ((p.error = ntt_r16_shape(b, false, count))) return p;
    } else {  // v1: one workgroup per (tile of 2^lt adjacent positions, column), LDS = tile + stage table[rows]
        b.family = NTT_V1;
        tile = (int)t.tile_log;
        if (tile < m_lo) tile = m_lo;
        b.lt = tile - m_lo;
        if (b.lt > m_hi) b.lt = m_hi;
        const uint32_t rows = 1u << m_lo, total = rows << b.lt;
        b.threads = total / 2 > 1024 ? 1024 : (total / 2 < 64 ? 64 : total / 2);
        if (b.threads > 512 && total <= 8192) b.threads = 512;
        b.lds = (size_t)total * 4 + (size_t)rows * 4;
        b.tiles = 1u << (m_hi - b.lt);
        b.grid_x = b.tiles;
        b.grid_y = (uint32_t)count;
    }
    return p;
}

// Columns per pass-A + pass-B round of a forward transform.  `count`: one round over all columns.  ntt_group_cols = g < count runs
// both passes on g columns at a time, so that pass B finds what pass A just wrote in the 256 MB Infinity Cache instead of HBM
// (SURVEY hard part 5; measured on the 2^22 LDE, DESIGN.md §4 "NTT traffic") — where both passes of a two-pass transform are on the
// radix-16 family.  (A refused group is returned as g: the caller reports the refusal of the plan it then makes.)
inline size_t ntt_forward_group(const NttTunables& t, int m, int expand_bits, int skip_bits, size_t count, bool aligned16) {
    const size_t g = (size_t)t.group_cols;
    if (!t.fast || g == 0 || g >= count) return count;
    const NttPlan p = ntt_plan(t, false, m, expand_bits, skip_bits, g, aligned16, false);
    return (p.error || (p.m_lo && p.a.r16() && p.b.r16())) ? g : count;
}

}  // namespace bx
