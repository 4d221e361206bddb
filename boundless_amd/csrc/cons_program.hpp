// cons_program.hpp — the compiled form of a constraint program (include/bx_program.h is the normative text): ONE instruction
// stream that the host executor (cons_program_host.cpp, the verifier's side) and the device kernel (cons_program.hip) both read; the
// compiler that writes it for all three program kinds is program_compile.cpp.
// Plain C++: the host half compiles without HIP.
//
// An instruction is two words:
//   w0 = opcode | dst << 8 | a << 16 | b << 24      dst, a, b: slot numbers (narrow or wide, as the opcode says)
//   w1 = c | imm << 8                               c: a third slot (AND_COND's inner); imm: table index (24 bits)
// Values live in two slot files: NARROW (one word, a base value) and WIDE (four words: an ext value or the tot of a mix var).
// dst may be a slot one of the sources is read from: an executor reads every source before it writes.
// Tables: `scal` = [globals (n_globals) | mix (4) | constants]: Montgomery words; an ext constant takes four consecutive ones.
//         `taps` = (col, back | group << 30) per entry of the program's tap list.
//         mix powers poly_mix^e, e < n_pows, canonical (mix_power_table).
// The stream is padded with NOPs to a multiple of CP_FETCH instructions: the kernel fetches that many at a time.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/bx_program.h"

namespace bx {

enum ConsOpcode : uint32_t {
    CP_NOP = 0,
    CP_LD_B,     // narrow[dst] = scal[imm]
    CP_LD_E,     // wide[dst] = scal[imm .. imm+3]
    CP_TAP,      // narrow[dst] = tap imm
    CP_ADD_BB,   // narrow[dst] = narrow[a] + narrow[b]
    CP_SUB_BB,
    CP_MUL_BB,
    CP_ADD_EB,   // wide[dst] = wide[a] + narrow[b]
    CP_SUB_EB,   // wide[dst] = wide[a] - narrow[b]
    CP_SUB_BE,   // wide[dst] = narrow[a] - wide[b]
    CP_MUL_EB,   // wide[dst] = wide[a] * narrow[b]
    CP_ADD_EE,   // wide[dst] = wide[a] + wide[b]
    CP_SUB_EE,
    CP_MUL_EE,
    CP_ZERO,     // wide[dst] = 0                                                    (TRUE)
    CP_EQZ_B,    // wide[dst] = wide[a] + pow[imm] * narrow[b]                       (AND_EQZ, base y)
    CP_EQZ_E,    // wide[dst] = wide[a] + pow[imm] * wide[b]                         (AND_EQZ, ext y)
    CP_COND_B,   // wide[dst] = wide[a] + (pow[imm] * wide[c]) * narrow[b]           (AND_COND, base cond)
    CP_COND_E,   // wide[dst] = wide[a] + (pow[imm] * wide[c]) * wide[b]             (AND_COND, ext cond)
    CP_ST,       // data column imm = narrow[a]                                      (SET; witness programs only, and last: no
                 //                                                                   existing stream or digest changes)
    // accumulate programs only ("Accumulate programs" of bx_program.h), appended for the same reason: a row's term of sequence imm
    CP_TSUM_B,   // run_ext[imm][r] = (narrow[b], 0, 0, 0), mults[imm][r] = narrow[a]  (SUM, base denominator)
    CP_TSUM_E,   // run_ext[imm][r] = wide[b],              mults[imm][r] = narrow[a]  (SUM, ext denominator)
    CP_TPROD_B,  // run_ext[imm][r] = (narrow[a], 0, 0, 0)                             (PROD, base factor)
    CP_TPROD_E,  // run_ext[imm][r] = wide[a]                                          (PROD, ext factor)
    // the denominator of a RATIO, appended last for the same reason; its numerator is a CP_TPROD_B/E with imm = the sequence.  imm = S + t
    // for the t-th of the R ratios: run_ext holds S + R sequences, [S, S + R) the denominators of sequences [S - R, S)
    CP_TDEN_B,   // run_ext[imm][r] = (narrow[a], 0, 0, 0)                             (RATIO, base denominator)
    CP_TDEN_E,   // run_ext[imm][r] = wide[a]                                          (RATIO, ext denominator)
    CP_OPCODES
};
constexpr uint32_t CP_FETCH = 4;  // instructions per fetch of the kernel (8 dwords)

inline uint32_t cp_w0(uint32_t op, uint32_t dst, uint32_t a, uint32_t b) { return op | dst << 8 | a << 16 | b << 24; }
inline uint32_t cp_w1(uint32_t c, uint32_t imm) { return c | imm << 8; }

// The opcode comments above in machine form: what each field of an instruction is, per opcode (cons_program_host.cpp: op_rules).
// A field the opcode does not use carries anything and is never looked at.
enum SlotClass : uint8_t { SLOT_NONE, SLOT_NARROW, SLOT_WIDE };
enum ImmClass : uint8_t {
    IMM_NONE,
    IMM_SCAL,    // one word of `scal`
    IMM_CONST4,  // four consecutive words of `scal`, all of them constants
    IMM_TAP,     // an entry of the tap list
    IMM_POW,     // a mix power
    IMM_SET,     // a data column below max_set
    IMM_SUM,     // a sequence in [0, sums)
    IMM_PROD,    // a sequence in [sums, S)
    IMM_DEN,     // a ratio's denominator: a sequence in [S, S + R)
};
enum ProgramKind : uint8_t { KIND_CONS = 1, KIND_WIT = 2, KIND_ACC = 4 };
struct OpRule {
    uint8_t dst, a, b, c;  // SlotClass
    uint8_t imm;           // ImmClass
    uint8_t kinds;         // the ProgramKinds whose streams may hold the opcode
};
const OpRule* op_rules();  // CP_OPCODES entries, indexed by opcode

// what a stream is held against: the program's own counts
struct StreamLimits {
    uint8_t kind;           // one ProgramKind
    uint32_t narrow, wide;  // the slot files
    size_t n_scal, consts_at;  // the size of `scal`, and where its constants begin
    const bx_cons_tap* taps;
    size_t n_taps;
    uint32_t tap_groups;    // a tap's group is below this
    uint32_t n_pows, max_set, sums, sequences, ratios;
};
// Does every instruction of `code` belong to the kind, and does every field its opcode uses stay inside its file or table?  Also
// false: slot files above BX_CONS_MAX_*, a length that is no whole number of fetches, a tap of an illegal group.
bool stream_fits(const std::vector<uint32_t>& code, const StreamLimits& lim);

}  // namespace bx

struct bx_cons_program {
    bx_cons_program_info info{};
    std::vector<uint32_t> code;    // 2 words per instruction, padded to CP_FETCH instructions
    std::vector<uint32_t> consts;  // Montgomery words: the tail of `scal`
    std::vector<bx_cons_tap> taps;
    uint32_t n_pows = 1;           // mix powers the stream names (at least 1: a table is never empty)
    uint32_t ret_slot = 0;         // the wide slot that holds mix[ret].tot at the end
    uint32_t max_col[3] = {0, 0, 0};  // 1 + the largest tap column per group (0 = the group is not named)
};

namespace bx {
// one multiplicity column of a witness program ("multiplicity columns" of bx_program.h), as create validated it
struct WitCount {
    uint32_t col = 0, bins = 0, rows = 0;
    std::vector<uint32_t> sources;
};
// one sort of a witness program ("sorted columns" of bx_program.h), as create validated it: bits.size() keys, the first of `sources`
struct WitSort {
    uint32_t rows = 0;
    std::vector<uint32_t> bits, sources, dests;
};
}  // namespace bx

// A compiled witness program ("Witness programs" of bx_program.h): the same two-word instructions, of the narrow opcodes CP_LD_B,
// CP_TAP, CP_ADD_BB, CP_SUB_BB, CP_MUL_BB and CP_ST only.  Its `scal` table is the constants alone (imm of CP_LD_B indexes `consts`).
struct bx_wit_program {
    bx_wit_program_info info{};
    std::vector<uint32_t> code;    // 2 words per instruction, padded to CP_FETCH instructions
    std::vector<uint32_t> consts;  // Montgomery words
    std::vector<bx_cons_tap> taps;
    std::vector<uint32_t> sets;    // the derived data columns, in the order of their SETs
    std::vector<bx_wit_global_cell> cells;
    uint32_t max_col[2] = {0, 0};  // 1 + the largest tap column per group (0 = the group is not named)
    uint32_t max_set = 0;          // 1 + the largest SET column
    std::vector<bx::WitCount> counts;  // run after the stream, in list order; not hashed, not emitted
    std::vector<bx::WitSort> sorts;    // run after the stream and before the counts, in list order; not hashed, not emitted
};

// A compiled accumulate program ("Accumulate programs" of bx_program.h): the instructions of a constraint program without the mix
// opcodes, plus the four term stores.  `scal` = [globals | mix (4) | consts], as for a constraint program.  CP_TAP's imm indexes `taps`;
// tap t reads kept column tap_kept[t], which is (group, col) = kept[tap_kept[t]].
struct bx_acc_program {
    bx_acc_program_info info{};
    std::vector<uint32_t> code;    // 2 words per instruction, padded to CP_FETCH instructions
    std::vector<uint32_t> consts;  // Montgomery words: the tail of `scal`
    std::vector<bx_cons_tap> taps;
    std::vector<uint32_t> tap_kept;  // per tap: its kept index
    std::vector<bx_cons_tap> kept;   // the distinct (group, col) of the tap list in order of first appearance (back unused, 0)
    uint32_t ratios = 0;             // R: sequences [S - R, S) are RATIOs (not in `info`, whose layout is fixed)
};

namespace bx {
// cons_program_host.cpp: stream_fits against the program's own counts, and the kind's header rules (ret_slot, the coherence of an
// accumulate program's kept / tap_kept / ratios).  The compiler's output always passes (the creates check it); every consumer of a
// program — the loads, the host executors, the emitters — calls this once and then trusts the stream.
bool program_fits(const bx_cons_program* p);
bool program_fits(const bx_wit_program* p);
bool program_fits(const bx_acc_program* p);
// cons_program_host.cpp: NULL, or the refusal (thread-local buffer, led by `who`) of a kept column that is not below its group's width: one
// text for bx_acc_program_run_host, bx_acc_program_keep and the composite table's create
const char* acc_program_check_widths(const std::vector<bx_cons_tap>& kept, const char* who, uint32_t w_code, uint32_t w_data);
// cons_program_host.cpp: NULL, or the refusal (in the caller's thread-local buffer, led by `who`) of a tap column (max_col, per group)
// or a SET column (max_set) that is not below its group's width: one text for bx_wit_program_run_host, bx_wit_program_run and the
// composite table's create
const char* wit_program_check_widths(const uint32_t max_col[2], uint32_t max_set, const char* who, uint32_t w_code, uint32_t w_data);
// cons_program_host.cpp: NULL, or the refusal (same buffer, led by `who`) of a count whose column or source is not below w_data, whose
// rows are above N = 2^po2, or whose bins are above N when rows == 0: the shape-dependent part of a count list, one text for the same
// three callers
const char* wit_program_check_counts(const std::vector<WitCount>& counts, const char* who, uint32_t po2, uint32_t w_data);
// cons_program_host.cpp: likewise for a sort whose rows are above N = 2^po2 or whose source or dest is not below w_data: the
// shape-dependent part of a sort list, one text for the same three callers
const char* wit_program_check_sorts(const std::vector<WitSort>& sorts, const char* who, uint32_t po2, uint32_t w_data);
}  // namespace bx
