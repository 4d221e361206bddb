/*
 * bx_lookup.h — the library's second built-in circuit: a range check proved with LogUp running sums.
 *
 * The circuits this backend stands in for do their range checks and memory arguments with a logarithmic-derivative argument:
 * every looked-up value a contributes 1 / (alpha - a) to a running sum, every table entry t contributes -m / (alpha - t) with m
 * the number of times it was looked up, and the sums close to zero exactly when every looked-up value is in the table.  This
 * circuit is the smallest complete instance: V values are split into two limbs each, every limb is looked up in the table
 * {0 .. B-1}, and the accumulate stage is ONE bx_logup_accumulate (bx_hal.h).  It plugs into the prover through the same
 * bx_circuit_ops table as the synthetic circuit (bx_circuit.h); commits, transcript, DEEP, FRI and the seal layout are shared.
 *
 * The lookup circuit (normative; N = 2^po2 rows, all row indices cyclic mod N)
 * ---------------------------------------------------------------------------
 *   words      splitmix64 and word(s,c,r) = splitmix64(s ^ (c << 32 | r)) >> 33, minus P if >= P, as in bx_prover.h.  Where a word
 *              is "reduced mod B" its integer value word(..) mod B is meant.  A cell "holds the value x" when its word is the
 *              Montgomery form x * 2^32 mod P; noise and filler cells hold word(..) itself as their Montgomery word.
 *   shape      po2 in [9, 24].  cons_terms and cons_degree are unused: normalize leaves 0 as 0 and refuses anything else.
 *              Z = min(1994, N/4) noise rows, A = N - Z active rows.  Limb width b = min(15, po2 - 1), B = 2^b: B <= N/2 <= A, and
 *              a value lo + B * hi is below 2^30 < P.
 *              V = min(floor((w_data - 1) / 3), floor((floor(w_accum / 4) - 1) / 2)) value columns; normalize refuses V = 0
 *              (w_data < 4 or w_accum < 12), w_code < 3 and V > 63.
 *   seeds      gseed_g = seed + (g+1) * 0x9E3779B97F4A7C15, nseed_g = noise_seed + (g+1) * 0x9E3779B97F4A7C15 (g = 1 data, 2 accum);
 *              noise_seed = splitmix64(seed ^ 0x5A4B4E4F49534521) unless given (bx_prove_segment_zk, bx_prover_set_noise_seed);
 *              cseed' = 0x4C4F4F4B55502121 ("LOOKUP!!"), a constant of this circuit's own: its control IDs differ from the synthetic
 *              circuit's at every shape.
 *   code       column 0 = first (1 at row 0, else 0); column 1 = last (1 at row A-1); column 2 = the table, t(r) = r for r < B, else
 *              0; column c >= 3 = word(cseed', c, r).  A function of (po2, w_code) alone.
 *   data       for j < V columns 3j, 3j+1, 3j+2 are v_j, lo_j, hi_j.  On the active rows r < A:
 *                  lo_j(r) = word(gseed_1, 3j+1, r) mod B;   hi_j(r) = word(gseed_1, 3j+2, r) mod B for even j, 0 for odd j;
 *                  v_j(r) = lo_j(r) + B * hi_j(r).
 *              (An odd value is small, as most of a real trace is: about V/2 * A lookups hit table entry 0.)
 *              Then the segment's cell records (below) overwrite cells.  Then column 3V, the multiplicity: for r < B, m(r) = the
 *              number of pairs (limb column 3j+1 or 3j+2, active row) whose cell holds the value t(r) = r; for B <= r < A, 0.
 *              Columns c > 3V: filler word(gseed_1, c, r).
 *              Noise rows r >= A: every column but the v_j holds word(nseed_1, c, r) (lo_j and every hi_j, the multiplicity
 *              and the filler alike), and v_j(r) = lo_j(r) + B * hi_j(r) in the field, so that constraint 1 holds on every row;
 *              the v_j are blinded through their limbs.  Noise rows are never counted in m.
 *   accum      drawn after the data commit: alpha (ext).  S = 2V + 1 sequences over all N rows:
 *                  s < 2V: the limb column a_s (a_0 = lo_0, a_1 = hi_0, a_2 = lo_1, ...; data column 3(s/2) + 1 + s%2),
 *                          denominator alpha - a_s(r), multiplicity 1;
 *                  s = 2V: the table, denominator alpha - t(r), multiplicity -m(r);
 *                  S_s(r) = sum_{i <= r} mult_s(i) / denom_s(i)   — what one bx_logup_accumulate with count = S writes.
 *              Component k of S_s is accum column 4s + k.  Columns c >= 4S: word(gseed_2 ^ (alpha.c0 << 32 | alpha.c1), c, r).
 *              The sums simply continue over the noise rows.
 *   taps       every column at Z; accum columns c < 4S also one row back (Z * w_N^-1).
 *   constraints, in mixing order (constraint i is weighted poly_mix^i; ext-valued constraints are mixed as ext elements)
 *              1. j < V :   v_j(r) - lo_j(r) - B * hi_j(r)                                                   = 0
 *              2. s < 2V :  (S_s(r) - (1 - first(r)) * S_s(r-1)) * (alpha - a_s(r)) - 1                      = 0
 *              3. table :   (S_2V(r) - (1 - first(r)) * S_2V(r-1)) * (alpha - t(r)) + m(r)                   = 0
 *              4. closing : last(r) * sum_{s <= 2V} S_s(r)                                                   = 0
 *              5. first(r) * (v_0(r) - g_0) = 0   and   last(r) * (v_0(r) - g_1) = 0
 *              3V + 4 constraints of degree <= 3, well inside the 4N check domain.
 *   globals    g_0 = v_0[0], g_1 = v_0[A-1] (Montgomery words), after the records were applied.
 *   check      as in bx_prover.h: sum_i poly_mix^i C_i(x) / ((3x)^N - 1) over x = w_4N^row, four ext planes = 16 check columns.
 *   segment    the "BXSYNSEG" stand-in header of bx_prover.h; the PAYLOAD is a list of cell records — what a preflight trace amounts
 *              to — of 12 bytes each: col u32 | row u32 | value u32, little endian.  Record k sets data cell (col, row) to the value
 *              `value`; when a cell is named more than once the last record wins.  They are applied after generation and before the
 *              multiplicities are counted; nothing is recomputed from a patched cell.  Each record needs col < 3V, row < A and
 *              value < P; a payload whose length is not a multiple of 12, more than BX_LOOKUP_MAX_RECORDS records, or a record outside
 *              those bounds is a witgen error.  A limb that does not hold a value below B is simply not counted.
 *              The prover does not judge the witness: it emits a seal and the verifier decides.
 */
#ifndef BX_LOOKUP_H
#define BX_LOOKUP_H
#include "bx_circuit.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BX_LOOKUP_MAX_VALUES 63      /* V */
#define BX_LOOKUP_MAX_LIMB_BITS 15   /* b <= 15: the table has at most 2^15 entries */
#define BX_LOOKUP_MAX_RECORDS 65536  /* cell records per segment */
#define BX_LOOKUP_RECORD_BYTES 12

/* The lookup circuit's table; provers are made with bx_prover_create_with_circuit, seals verified with
 * bx_verify_segment_with_circuit / _with_context[_hashfn].  A prover of this circuit keeps its code commitment like one of the
 * synthetic circuit (ctx tunable code_commit_once): the code group is shape-only by construction. */
const bx_circuit_ops* bx_lookup_circuit(void);

/* The lookup circuit's control ID for (po2, w_code) under a named hash suite ("poseidon2" or "sha-256"; anything else is refused),
 * computed on the HOST from the definition (code columns -> interpolation -> evaluation on the coset 3<w_4N> -> row hashes -> tree)
 * and cached per (po2, w_code, suite).  No generated table.  bx_lookup_circuit()->check_code uses it for Poseidon2; under "sha-256"
 * the verifier uses it when it is given no context. */
const char* bx_lookup_control_id_host_hashfn(uint32_t po2, uint32_t w_code, const char* hashfn, uint32_t id_out[8]);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
