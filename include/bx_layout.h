/*
 * bx_layout.h — trace layouts: the BASE of a circuit from data.
 *
 * A circuit made of programs (bx_program.h) takes its taps, eval_check and verifier from a constraint program, its derived columns
 * from a witness program and its running sums from an accumulate program; what is left — the code group, the free cells of the data
 * group, the noise rows, the accum filler, the public words and check_code — came from a hand-written base table.  A trace layout
 * describes that rest in data: (a) the code columns as a function of the shape, (b) where each free data cell comes from in the
 * segment's row-major records, (c) the noise rows.  Compiled, it IS a base table: bx_cons_circuit_create(bx_trace_layout_ops(l), prog, ..)
 * is a whole circuit with no C++ or Python callback behind it, and a verifier can compute its control ID on the host.
 * Upstream's witgen starts with "preflight trace -> witgen kernels" (bx_circuit.h, witgen); bx_trace_layout_place is that step.
 *
 * Trace layouts (normative)
 * -------------------------
 *   N = 2^po2 rows.  Z = min(noise_rows, N/4) noise rows, A = N - Z active rows.  splitmix64 and word(s, c, r) are those of
 *   bx_prover.h.  A cell "holds the value x" when its word is the Montgomery form x * 2^32 mod P.
 *
 *   code       the code group has exactly n_code columns (w_code == n_code) and is a function of (po2, layout) only.  Cell (c, r) of
 *              column c with (kind, a, b):
 *                CONST     holds the value a (a < P)
 *                FIRST     holds 1 at row 0, else 0
 *                LAST      holds 1 at row A - 1 - a, else 0
 *                ACTIVE    holds 1 for r < A - a, else 0
 *                ROW       holds the value r for r < min(N, a ? a : N), else 0   (the lookup circuit's table column)
 *                PERIODIC  holds the value table[b + (r mod 2^a)], with a <= 12 and b + 2^a <= n_table
 *                WORD      is the Montgomery word word(a | b << 32, c, r)          (the built-in circuits' random selector columns)
 *              LAST or ACTIVE with a >= A at a given po2 is refused where the shape is known (normalize, the host fills, the device
 *              entries); it is not wrapped.
 *   data       the segment is the "BXSYNSEG" header of bx_prover.h (28 bytes) followed by a payload of exactly R records of `stride`
 *              little-endian u32 words, 0 <= R <= A.  A field (col, word, shift, bits, pad) puts into data cell (col, r), for r < R,
 *              the value (record_r[word] >> shift) & (2^bits - 1); for R <= r < A the cell holds the value pad.  bits is in 1..30, so
 *              every value is below P and no record can be out of range: the prover does not judge the witness.  shift + bits <= 32,
 *              word < stride, pad < 2^bits.  A record word may feed any number of fields; a column is named by at most one field.  A
 *              column below w_data that no field names holds 0 on the active rows.  Rows r >= A of EVERY data column hold
 *              word(nseed_1, c, r), nseed_1 = noise_seed + 2 * 0x9E3779B97F4A7C15; the noise seed is the one given through
 *              set_noise_seed, else splitmix64(seed ^ 0x5A4B4E4F49534521).
 *   globals    n_globals zero words.  A witness program's global cells override them (bx_cons_circuit_set_witness).
 *   accum      every column is filler word(gseed_2 ^ (mix.c0 << 32 | mix.c1), c, r), gseed_2 = seed + 3 * 0x9E3779B97F4A7C15.  An
 *              accumulate program overwrites columns [0, 4 S).
 *   witgen     refuses, each by its own message and with nothing written: a payload whose length is not a multiple of 4 * stride;
 *              R > A.
 *   the table  normalize: cons_terms and cons_degree 0 stay 0, anything else is refused; w_code must equal n_code; w_data must
 *              exceed the largest field column; LAST / ACTIVE are checked against A; po2 in [1, 24].  check_code computes the control
 *              ID on the host (Poseidon2; cached per layout and po2) — under "sha-256" an explicit verifier context is needed, as for
 *              any plug-in.  The layout's own table is a base, not a circuit: taps answers {0} for every column, eval_check and
 *              constraints_at return a message that names bx_cons_circuit_create.
 *
 * Out of scope: values of 31 or 32 bits (split them into limbs with shift / bits); free cells computed from other free cells
 * (derived columns: a witness program); keeping the code commitment across proofs (code_commit_once needs a new member of
 * bx_circuit_ops, which carries no size field).
 */
#ifndef BX_LAYOUT_H
#define BX_LAYOUT_H
#include "bx_circuit.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BX_LAYOUT_MAX_STRIDE 128       /* words per record */
#define BX_LAYOUT_MAX_PERIOD_BITS 12   /* PERIODIC: a <= 12 */
#define BX_LAYOUT_MAX_FIELD_BITS 30

enum bx_layout_code_kind {
    BX_LAYOUT_CONST = 0,
    BX_LAYOUT_FIRST = 1,
    BX_LAYOUT_LAST = 2,
    BX_LAYOUT_ACTIVE = 3,
    BX_LAYOUT_ROW = 4,
    BX_LAYOUT_PERIODIC = 5,
    BX_LAYOUT_WORD = 6
};

typedef struct bx_layout_code_col {
    uint32_t kind, a, b;
} bx_layout_code_col;
typedef struct bx_layout_field {
    uint32_t col, word, shift, bits, pad;
} bx_layout_field;
typedef struct bx_trace_layout_desc {
    const bx_layout_code_col* code;
    uint32_t n_code; /* w_code == n_code exactly */
    const uint32_t* table;
    uint32_t n_table; /* values of PERIODIC columns, each < P */
    const bx_layout_field* fields;
    uint32_t n_fields;
    uint32_t stride;     /* words per record, 1 .. BX_LAYOUT_MAX_STRIDE */
    uint32_t noise_rows; /* 0 = no ZK rows; the built-in circuits use 1994 */
    uint32_t n_globals;  /* <= BX_MAX_GLOBALS */
} bx_trace_layout_desc;
typedef struct bx_trace_layout_info {
    uint32_t n_code, n_table, n_fields, stride, noise_rows, n_globals;
    uint32_t min_w_data; /* the largest field column + 1 (0 without fields) */
} bx_trace_layout_info;

typedef struct bx_trace_layout bx_trace_layout;
typedef struct bx_trace_layout_dev bx_trace_layout_dev;

/* Compiles a description (copied: the caller's arrays are free afterwards).  A null argument is refused first; then the FIRST of
 * these rules that any element breaks is the refusal, each rule looked at over the whole description before the next, each with a
 * message of its own that starts with "trace_layout: ":
 *    1. a code column of unknown kind                   "code column %u: unknown kind %u"
 *    2. a out of range for its kind                     "code column %u: CONST value %u is not below P" /
 *                                                       "code column %u: PERIODIC period 2^%u is above 2^12"
 *    3. a PERIODIC window outside the table             "code column %u: PERIODIC window [%u, %llu) is outside the table of %u values"
 *    4. a table value >= P                              "table value %u (%u) is not below P"
 *    5. stride 0 or above 128                           "stride %u is not in 1 .. 128"
 *    6. a field whose word is >= stride                 "field %u: word %u is not below the stride %u"
 *    7. bits 0 or above 30                              "field %u: bits %u is not in 1 .. 30"
 *    8. shift + bits above 32                           "field %u: shift %u + bits %u is above 32"
 *    9. pad >= 2^bits                                   "field %u: pad %u is not below 2^%u"
 *   10. a column named twice                            "field %u: column %u is named a second time (first by field %u)"
 *   11. n_code 0 or >= 65536                            "n_code %u is not in 1 .. 65535"
 *   12. a field column >= 65535                         "field %u: column %u is not below 65535"
 *   13. n_globals above BX_MAX_GLOBALS                  "n_globals %u is above BX_MAX_GLOBALS = 64"
 * Messages live in thread-local storage. */
const char* bx_trace_layout_create(const bx_trace_layout_desc* desc, bx_trace_layout** out);
void bx_trace_layout_destroy(bx_trace_layout* layout);
const char* bx_trace_layout_info_get(const bx_trace_layout* layout, bx_trace_layout_info* out);
/* The layout as a base table for bx_cons_circuit_create (the table lives in the layout and must outlive every circuit and prover
 * made from it). */
const bx_circuit_ops* bx_trace_layout_ops(bx_trace_layout* layout);

/* Host fills (plain C++, no ctx, no GPU): the definition, what the device entries are compared with.
 * code_out: n_code columns of N words, column-major.  po2 in [1, 24]. */
const char* bx_trace_layout_code_host(const bx_trace_layout* layout, uint32_t po2, uint32_t* code_out);
/* data_out: w_data columns of N words.  segment = header + payload (segment_len bytes); the header's po2 must be po2.
 * noise_seed NULL = derived from the segment's seed.  A refusal leaves data_out untouched. */
const char* bx_trace_layout_data_host(const bx_trace_layout* layout, uint32_t po2, const uint8_t* segment, size_t segment_len,
                                      const uint64_t* noise_seed, uint32_t* data_out, uint32_t w_data);
/* The control ID of a circuit over this layout at po2 in [9, 24] under a named hash suite ("poseidon2" or "sha-256"): the Merkle
 * root of the committed code group, computed on the host from the definition and cached per (layout, po2, suite). */
const char* bx_trace_layout_control_id_host_hashfn(const bx_trace_layout* layout, uint32_t po2, const char* hashfn, uint32_t id_out[8]);

/* Device entries, so that the kernels can be used and tested outside a proof.  Non-blocking: they enqueue on the ctx's stream.
 * Each refuses by message, with nothing touched, a size mismatch, overlapping operands and a layout loaded on another ctx.  A
 * loaded layout that is not unloaded is released by bx_free; a second unload, or one after bx_free, is answered by message. */
const char* bx_trace_layout_load(bx_ctx* ctx, const bx_trace_layout* layout, bx_trace_layout_dev** out);
const char* bx_trace_layout_unload(bx_trace_layout_dev* dev);
/* code: N x n_code words */
const char* bx_trace_layout_code(bx_ctx* ctx, bx_trace_layout_dev* dev, uint32_t po2, bx_buf code);
/* The free cells from the segment's bytes in HBM: segment_dev holds ceil(segment_len / 4) words or more, header included (what
 * bx_circuit_ops::witgen is handed); data: N x w_data words.  The seed is not read from the device: noise_seed is the noise seed
 * itself (not nseed_1). */
const char* bx_trace_layout_place(bx_ctx* ctx, bx_trace_layout_dev* dev, uint32_t po2, bx_buf segment_dev, size_t segment_len, uint64_t noise_seed,
                                  bx_buf data, uint32_t w_data);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
