// program_fits_check.cpp — stand-alone checker of the operand table and the one stream check of the three program kinds
// (csrc/cons_program.hpp: op_rules, program_fits), built with -fsanitize=address,undefined by tests/test_program_fits_cpu.py and run
// as a process of its own.
//
// For each kind one small program that holds every opcode of the kind is compiled.  Then, one field of one instruction at a time:
//   every field the table calls used gets the smallest bad value — a slot = the file's count, and 255; imm = the table's size; for
//   the sequence classes one below and one past the range; for an ext constant also one word below the constants — and
//   program_fits must say no;
//   every opcode of a foreign kind, CP_OPCODES and 255 in place of an instruction must be refused;
//   every unused field of every instruction set to all ones, all at once, must still be accepted.
// The bad values are worked out here from the program's own counts, not from stream_fits.  Last, every consumer that takes a program
// without a ctx — both host executors, constraints_at, both emitters — gets a corrupt stream of its kind and must answer "corrupt
// instruction stream" with no sanitizer report; constraints_at with dst = 255 is the one that used to overrun its slot arrays.
#include <stdio.h>
#include <string.h>

#include <utility>
#include <vector>

#include "bx_program.h"
#include "cons_program.hpp"

using namespace bx;

static int g_bad = 0;
#define EXPECT(cond, ...)        \
    do {                         \
        if (!(cond)) {           \
            printf(__VA_ARGS__); \
            printf("\n");        \
            ++g_bad;             \
        }                        \
    } while (0)

// the value steps every kind with ext values can hold: fp vars 0 .. 13, one of each base / ext opcode
static const bx_cons_step kValues[] = {
    {BX_CONS_CONST, 3, 0, 0, 0},       // 0  LD_B (a constant)
    {BX_CONS_GET, 0, 0, 0, 0},         // 1  TAP
    {BX_CONS_GET_GLOBAL, 0, 0, 0, 0},  // 2  LD_B (a global)
    {BX_CONS_CONST_EXT, 1, 2, 3, 4},   // 3  LD_E
    {BX_CONS_ADD, 0, 1, 0, 0},         // 4  ADD_BB
    {BX_CONS_SUB, 4, 2, 0, 0},         // 5  SUB_BB
    {BX_CONS_MUL, 5, 0, 0, 0},         // 6  MUL_BB
    {BX_CONS_ADD, 3, 6, 0, 0},         // 7  ADD_EB
    {BX_CONS_SUB, 7, 6, 0, 0},         // 8  SUB_EB
    {BX_CONS_SUB, 6, 8, 0, 0},         // 9  SUB_BE
    {BX_CONS_MUL, 9, 0, 0, 0},         // 10 MUL_EB
    {BX_CONS_ADD, 10, 3, 0, 0},        // 11 ADD_EE
    {BX_CONS_SUB, 11, 3, 0, 0},        // 12 SUB_EE
    {BX_CONS_MUL, 12, 3, 0, 0},        // 13 MUL_EE
};
static const bx_cons_tap kTaps[] = {{1, 0, 1}, {0, 1, 0}};

// what the bad values of one program are made from
struct Counts {
    uint8_t kind;
    uint32_t narrow, wide;
    uint32_t n_scal, consts_at, n_taps, n_pows, max_set, sums, S, R;
};

static uint32_t field(const std::vector<uint32_t>& code, size_t pc, int f) {  // 0 dst, 1 a, 2 b, 3 c, 4 imm
    const uint32_t w0 = code[pc], w1 = code[pc + 1];
    return f == 0 ? (w0 >> 8) & 0xFFu : f == 1 ? (w0 >> 16) & 0xFFu : f == 2 ? w0 >> 24 : f == 3 ? w1 & 0xFFu : w1 >> 8;
}
static void set_field(std::vector<uint32_t>& code, size_t pc, int f, uint32_t v) {
    if (f < 3) code[pc] = (code[pc] & ~(0xFFu << (8 * (f + 1)))) | v << (8 * (f + 1));
    else if (f == 3) code[pc + 1] = (code[pc + 1] & ~0xFFu) | v;
    else code[pc + 1] = (code[pc + 1] & 0xFFu) | v << 8;
}

// `code` is the program's own stream, `fits` asks program_fits about the program as it stands
template <class Fits>
static void sweep(const char* who, std::vector<uint32_t>& code, const Counts& n, Fits fits) {
    static const char* const kField[] = {"dst", "a", "b", "c", "imm"};
    const OpRule* const rules = op_rules();
    const std::vector<uint32_t> intact = code;
    EXPECT(fits(), "%s: the compiled program does not pass program_fits", who);
    // every opcode of the kind is there
    for (uint32_t op = 0; op < CP_OPCODES; ++op) {
        if (!(rules[op].kinds & n.kind)) continue;
        bool found = false;
        for (size_t pc = 0; pc < code.size(); pc += 2) found |= (code[pc] & 0xFFu) == op;
        EXPECT(found, "%s: the program holds no opcode %u: the sweep would not reach its row", who, op);
    }
    long bad_values = 0;
    for (size_t pc = 0; pc < intact.size(); pc += 2) {
        const uint32_t op = intact[pc] & 0xFFu;
        const OpRule& r = rules[op];
        const uint8_t cls[4] = {r.dst, r.a, r.b, r.c};
        std::vector<std::pair<int, uint32_t>> bad;  // (field, value)
        for (int f = 0; f < 4; ++f) {
            if (cls[f] == SLOT_NONE) continue;
            bad.push_back({f, cls[f] == SLOT_NARROW ? n.narrow : n.wide});
            bad.push_back({f, 255u});
        }
        switch (r.imm) {
        case IMM_SCAL: bad.push_back({4, n.n_scal}); break;
        case IMM_CONST4:
            bad.push_back({4, n.n_scal - 3});  // the fourth word is past the table
            bad.push_back({4, n.n_scal});
            bad.push_back({4, n.consts_at - 1});  // a word of the globals or the mix, not a constant
            break;
        case IMM_TAP: bad.push_back({4, n.n_taps}); break;
        case IMM_POW: bad.push_back({4, n.n_pows}); break;
        case IMM_SET: bad.push_back({4, n.max_set}); break;
        case IMM_SUM: bad.push_back({4, n.sums}); break;
        case IMM_PROD:
            bad.push_back({4, n.sums - 1});
            bad.push_back({4, n.S});
            break;
        case IMM_DEN:
            bad.push_back({4, n.S - 1});
            bad.push_back({4, n.S + n.R});
            break;
        default: break;
        }
        for (const auto& fv : bad) {
            set_field(code, pc, fv.first, fv.second);
            EXPECT(field(code, pc, fv.first) == fv.second, "%s: the checker's own set_field is wrong", who);
            EXPECT(!fits(), "%s: instruction %zu (opcode %u) with %s = %u was accepted", who, pc / 2, op, kField[fv.first], fv.second);
            code = intact;
            ++bad_values;
        }
        // a foreign opcode, and no opcode at all, in this instruction's place
        for (uint32_t other = 0; other <= 255; ++other) {
            if (other < CP_OPCODES && (rules[other].kinds & n.kind)) continue;
            if (other > CP_OPCODES && other < 255) continue;
            code[pc] = (code[pc] & ~0xFFu) | other;
            EXPECT(!fits(), "%s: opcode %u in place of instruction %zu was accepted", who, other, pc / 2);
            code = intact;
        }
    }
    // every unused field of every instruction at once
    for (size_t pc = 0; pc < code.size(); pc += 2) {
        const OpRule& r = rules[code[pc] & 0xFFu];
        const uint8_t cls[4] = {r.dst, r.a, r.b, r.c};
        for (int f = 0; f < 4; ++f)
            if (cls[f] == SLOT_NONE) set_field(code, pc, f, 255u);
        if (r.imm == IMM_NONE) set_field(code, pc, 4, 0xFFFFFFu);
    }
    EXPECT(code != intact, "%s: no unused field was found", who);
    EXPECT(fits(), "%s: a stream whose unused fields are all ones was refused", who);
    code = intact;
    EXPECT(fits(), "%s: the restored stream is refused", who);
    printf("%s: %zu instructions, %ld bad values refused\n", who, intact.size() / 2, bad_values);
}

static bool is_corrupt(const char* e) { return e && strstr(e, "corrupt instruction stream"); }

// the first instruction of opcode `op`
static size_t find_op(const std::vector<uint32_t>& code, uint32_t op) {
    for (size_t pc = 0; pc < code.size(); pc += 2)
        if ((code[pc] & 0xFFu) == op) return pc;
    printf("the stream holds no opcode %u\n", op);
    ++g_bad;
    return 0;
}

static const char* zero_tap(const void*, int, uint32_t, int, uint32_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0u;
    return nullptr;
}

static void cons_kind() {
    std::vector<bx_cons_step> steps(kValues, kValues + 14);
    steps.push_back({BX_CONS_TRUE, 0, 0, 0, 0});          // mix 0: ZERO
    steps.push_back({BX_CONS_AND_EQZ, 0, 6, 0, 0});       // mix 1: EQZ_B
    steps.push_back({BX_CONS_AND_EQZ, 1, 13, 0, 0});      // mix 2: EQZ_E
    steps.push_back({BX_CONS_AND_COND, 2, 1, 1, 0});      // mix 3: COND_B
    steps.push_back({BX_CONS_AND_COND, 3, 13, 2, 0});     // mix 4: COND_E
    bx_cons_program_desc d{steps.data(), steps.size(), kTaps, 2, 1, 4};
    bx_cons_program* p = nullptr;
    if (const char* e = bx_cons_program_create(&d, &p)) {
        printf("cons: create: %s\n", e);
        ++g_bad;
        return;
    }
    const uint32_t at = p->info.n_globals + 4;
    const Counts n{KIND_CONS, p->info.narrow, p->info.wide, at + (uint32_t)p->consts.size(), at, (uint32_t)p->taps.size(), p->n_pows, 0, 0, 0, 0};
    sweep("cons", p->code, n, [&] { return program_fits(p); });
    // the header rules
    const uint32_t ret = p->ret_slot;
    p->ret_slot = p->info.wide;
    EXPECT(!program_fits(p), "cons: ret_slot = wide was accepted");
    p->ret_slot = ret;
    p->taps[0].group = 3;
    EXPECT(!program_fits(p), "cons: tap group 3 was accepted");
    p->taps[0].group = kTaps[0].group;
    const std::vector<uint32_t> intact = p->code;
    p->code.resize(p->code.size() - 2);
    EXPECT(!program_fits(p), "cons: a stream that is no whole number of fetches was accepted");
    p->code = intact;
    EXPECT(program_fits(p), "cons: the restored program is refused");

    // the consumers: a wide destination of 255 (constraints_at's arrays have BX_CONS_MAX_WIDE entries), a power past the table
    const uint32_t pm[4] = {5, 6, 7, 8}, mix[4] = {1, 2, 3, 4}, globals[1] = {9};
    const bx_tap_reader reader{nullptr, zero_tap};
    uint32_t out[4];
    EXPECT(bx_cons_program_constraints_at(p, &reader, pm, mix, globals, out) == nullptr, "cons: constraints_at refuses the intact program");
    size_t need = 0;
    EXPECT(bx_cons_program_emit_hip(p, nullptr, 0, &need) == nullptr && need > 100, "cons: the emitter refuses the intact program");
    const struct {
        uint32_t op;
        int f;
        uint32_t v;
    } cases[] = {{CP_MUL_EE, 0, 255u}, {CP_MUL_BB, 0, 255u}, {CP_COND_E, 3, 255u}, {CP_EQZ_B, 4, p->n_pows}, {CP_LD_E, 4, n.n_scal - 3}, {CP_TAP, 4, n.n_taps}};
    for (const auto& cs : cases) {
        set_field(p->code, find_op(p->code, cs.op), cs.f, cs.v);
        EXPECT(is_corrupt(bx_cons_program_constraints_at(p, &reader, pm, mix, globals, out)), "cons: constraints_at took opcode %u with field %d = %u", cs.op, cs.f, cs.v);
        need = 77;
        EXPECT(is_corrupt(bx_cons_program_emit_hip(p, nullptr, 0, &need)) && need == 0, "cons: the emitter took opcode %u with field %d = %u", cs.op, cs.f, cs.v);
        p->code = intact;
    }
    bx_cons_program_destroy(p);
}

static void wit_kind() {
    const bx_cons_step steps[] = {{BX_CONS_GET, 0, 0, 0, 0}, {BX_CONS_GET, 1, 0, 0, 0}, {BX_CONS_CONST, 5, 0, 0, 0}, {BX_CONS_ADD, 0, 1, 0, 0},
                                  {BX_CONS_SUB, 3, 2, 0, 0}, {BX_CONS_MUL, 4, 0, 0, 0}, {BX_CONS_SET, 3, 5, 0, 0}};
    bx_wit_program_desc d{steps, 7, kTaps, 2, nullptr, 0};
    bx_wit_program* p = nullptr;
    if (const char* e = bx_wit_program_create(&d, &p)) {
        printf("wit: create: %s\n", e);
        ++g_bad;
        return;
    }
    const Counts n{KIND_WIT, p->info.narrow, 0, (uint32_t)p->consts.size(), 0, (uint32_t)p->taps.size(), 0, p->max_set, 0, 0, 0};
    sweep("wit", p->code, n, [&] { return program_fits(p); });
    p->taps[0].group = 2;
    EXPECT(!program_fits(p), "wit: tap group 2 was accepted");
    p->taps[0].group = kTaps[0].group;

    const std::vector<uint32_t> intact = p->code;
    constexpr uint32_t PO2 = 2, N = 1u << PO2, W_CODE = 2, W_DATA = 4;
    std::vector<uint32_t> code(W_CODE * N, 1u), data(W_DATA * N, 2u);  // exact-size heap blocks: ASan watches their ends
    EXPECT(bx_wit_program_run_host(p, PO2, code.data(), W_CODE, data.data(), W_DATA) == nullptr, "wit: run_host refuses the intact program");
    size_t need = 0;
    EXPECT(bx_wit_program_emit_hip(p, nullptr, 0, &need) == nullptr && need > 100, "wit: the emitter refuses the intact program");
    const struct {
        uint32_t op;
        int f;
        uint32_t v;
    } cases[] = {{CP_MUL_BB, 0, 255u}, {CP_ADD_BB, 2, p->info.narrow}, {CP_ST, 1, 255u}, {CP_ST, 4, p->max_set}, {CP_TAP, 4, n.n_taps}, {CP_LD_B, 4, n.n_scal}};
    for (const auto& cs : cases) {
        set_field(p->code, find_op(p->code, cs.op), cs.f, cs.v);
        EXPECT(is_corrupt(bx_wit_program_run_host(p, PO2, code.data(), W_CODE, data.data(), W_DATA)), "wit: run_host took opcode %u with field %d = %u", cs.op, cs.f, cs.v);
        need = 77;
        EXPECT(is_corrupt(bx_wit_program_emit_hip(p, nullptr, 0, &need)) && need == 0, "wit: the emitter took opcode %u with field %d = %u", cs.op, cs.f, cs.v);
        p->code = intact;
    }
    bx_wit_program_destroy(p);
}

static void acc_kind() {
    std::vector<bx_cons_step> steps(kValues, kValues + 14);
    steps.push_back({BX_CONS_SUM, 0, 1, 6, 0});     // TSUM_B
    steps.push_back({BX_CONS_SUM, 1, 1, 13, 0});    // TSUM_E
    steps.push_back({BX_CONS_PROD, 2, 6, 0, 0});    // TPROD_B
    steps.push_back({BX_CONS_PROD, 3, 13, 0, 0});   // TPROD_E
    steps.push_back({BX_CONS_RATIO, 4, 6, 4, 0});   // TPROD_B, TDEN_B
    steps.push_back({BX_CONS_RATIO, 5, 13, 7, 0});  // TPROD_E, TDEN_E
    bx_acc_program_desc d{steps.data(), steps.size(), kTaps, 2, 1};
    bx_acc_program* p = nullptr;
    if (const char* e = bx_acc_program_create(&d, &p)) {
        printf("acc: create: %s\n", e);
        ++g_bad;
        return;
    }
    const uint32_t at = p->info.n_globals + 4;
    const Counts n{KIND_ACC,          p->info.narrow, p->info.wide, at + (uint32_t)p->consts.size(), at, (uint32_t)p->taps.size(), 0, 0,
                   p->info.sums, p->info.sequences, p->ratios};
    EXPECT(n.sums == 2 && n.S == 6 && n.R == 2, "acc: the program is not the one this checker was written for");
    sweep("acc", p->code, n, [&] { return program_fits(p); });
    // the header rules
    p->ratios = n.S - n.sums + 1;
    EXPECT(!program_fits(p), "acc: more ratios than products was accepted");
    p->ratios = n.R;
    p->tap_kept[0] = (uint32_t)p->kept.size();
    EXPECT(!program_fits(p), "acc: a tap of a kept column past the list was accepted");
    p->tap_kept[0] = 0;
    p->kept[0].group = 2;
    EXPECT(!program_fits(p), "acc: a kept column of group 2 was accepted");
    p->kept[0].group = kTaps[0].group;
    EXPECT(program_fits(p), "acc: the restored program is refused");

    const std::vector<uint32_t> intact = p->code;
    constexpr uint32_t PO2 = 2, N = 1u << PO2, W_CODE = 2, W_DATA = 1;
    std::vector<uint32_t> code(W_CODE * N, 1u), data(W_DATA * N, 2u), accum(4 * n.S * N, 0u);
    const uint32_t mix[4] = {1, 2, 3, 4}, globals[1] = {9};
    const auto run = [&] { return bx_acc_program_run_host(p, PO2, code.data(), W_CODE, data.data(), W_DATA, globals, mix, accum.data(), 4 * n.S); };
    EXPECT(run() == nullptr, "acc: run_host refuses the intact program");
    const struct {
        uint32_t op;
        int f;
        uint32_t v;
    } cases[] = {{CP_MUL_EE, 0, 255u},   {CP_MUL_EE, 1, p->info.wide}, {CP_TSUM_E, 2, 255u},       {CP_TSUM_B, 4, n.sums},
                 {CP_TPROD_E, 4, n.S}, {CP_TDEN_B, 4, n.S + n.R},    {CP_LD_E, 4, n.n_scal - 3}, {CP_TAP, 4, n.n_taps}};
    for (const auto& cs : cases) {
        set_field(p->code, find_op(p->code, cs.op), cs.f, cs.v);
        EXPECT(is_corrupt(run()), "acc: run_host took opcode %u with field %d = %u", cs.op, cs.f, cs.v);
        p->code = intact;
    }
    bx_acc_program_destroy(p);
}

int main() {
    cons_kind();
    wit_kind();
    acc_kind();
    if (g_bad) return printf("%d checks failed\n", g_bad), 1;
    printf("program_fits_check ok\n");
    return 0;
}
