// cons_program_host.cpp — the host side of a COMPILED program of any of the three kinds (include/bx_program.h is the normative text;
// program_compile.cpp makes the compiled form of cons_program.hpp): the host executors of the stream — constraints_at over Fp4 for
// the verifier, and the row executors of witness and accumulate programs, which share one instruction body (host_exec, the host twin
// of the device's cp_exec) — the shape checks the host and device paths say in one text, and the small getters of the C ABI.
// No HIP: this translation unit compiles with plain g++ (the stand-alone checkers under tests/ run it under sanitizers).
#include <string.h>

#include <algorithm>

#include "fp.hpp"
#include "program_internal.hpp"

namespace bx {

// a function, not an object: the library's build compiles this file as HIP, where a namespace-scope constant would be emitted for the
// device too
const OpRule* op_rules() {
    constexpr uint8_t _ = SLOT_NONE, N = SLOT_NARROW, W = SLOT_WIDE, ALL = KIND_CONS | KIND_WIT | KIND_ACC, EXT = KIND_CONS | KIND_ACC;
    static constexpr OpRule rules[] = {
        //           dst a  b  c  imm         kinds
        /* NOP     */ {_, _, _, _, IMM_NONE, ALL},
        /* LD_B    */ {N, _, _, _, IMM_SCAL, ALL},
        /* LD_E    */ {W, _, _, _, IMM_CONST4, EXT},
        /* TAP     */ {N, _, _, _, IMM_TAP, ALL},
        /* ADD_BB  */ {N, N, N, _, IMM_NONE, ALL},
        /* SUB_BB  */ {N, N, N, _, IMM_NONE, ALL},
        /* MUL_BB  */ {N, N, N, _, IMM_NONE, ALL},
        /* ADD_EB  */ {W, W, N, _, IMM_NONE, EXT},
        /* SUB_EB  */ {W, W, N, _, IMM_NONE, EXT},
        /* SUB_BE  */ {W, N, W, _, IMM_NONE, EXT},
        /* MUL_EB  */ {W, W, N, _, IMM_NONE, EXT},
        /* ADD_EE  */ {W, W, W, _, IMM_NONE, EXT},
        /* SUB_EE  */ {W, W, W, _, IMM_NONE, EXT},
        /* MUL_EE  */ {W, W, W, _, IMM_NONE, EXT},
        /* ZERO    */ {W, _, _, _, IMM_NONE, KIND_CONS},
        /* EQZ_B   */ {W, W, N, _, IMM_POW, KIND_CONS},
        /* EQZ_E   */ {W, W, W, _, IMM_POW, KIND_CONS},
        /* COND_B  */ {W, W, N, W, IMM_POW, KIND_CONS},
        /* COND_E  */ {W, W, W, W, IMM_POW, KIND_CONS},
        /* ST      */ {_, N, _, _, IMM_SET, KIND_WIT},
        /* TSUM_B  */ {_, N, N, _, IMM_SUM, KIND_ACC},
        /* TSUM_E  */ {_, N, W, _, IMM_SUM, KIND_ACC},
        /* TPROD_B */ {_, N, _, _, IMM_PROD, KIND_ACC},
        /* TPROD_E */ {_, W, _, _, IMM_PROD, KIND_ACC},
        /* TDEN_B  */ {_, N, _, _, IMM_DEN, KIND_ACC},
        /* TDEN_E  */ {_, W, _, _, IMM_DEN, KIND_ACC},
    };
    static_assert(sizeof rules / sizeof rules[0] == CP_OPCODES, "one row per opcode, in the order of ConsOpcode");
    return rules;
}

bool stream_fits(const std::vector<uint32_t>& code, const StreamLimits& lim) {
    if (lim.narrow > BX_CONS_MAX_NARROW || lim.wide > BX_CONS_MAX_WIDE || code.size() % (2 * CP_FETCH)) return false;
    for (size_t t = 0; t < lim.n_taps; ++t)
        if (lim.taps[t].group >= lim.tap_groups) return false;
    const OpRule* const rules = op_rules();
    const auto slot = [&](uint8_t cls, uint32_t s) { return cls == SLOT_NONE || s < (cls == SLOT_NARROW ? lim.narrow : lim.wide); };
    for (size_t pc = 0; pc < code.size(); pc += 2) {
        const uint32_t w0 = code[pc], w1 = code[pc + 1], op = w0 & 0xFFu;
        const size_t imm = w1 >> 8;
        if (op >= CP_OPCODES || !(rules[op].kinds & lim.kind)) return false;
        const OpRule& r = rules[op];
        if (!slot(r.dst, (w0 >> 8) & 0xFFu) || !slot(r.a, (w0 >> 16) & 0xFFu) || !slot(r.b, w0 >> 24) || !slot(r.c, w1 & 0xFFu)) return false;
        bool ok = true;
        switch (r.imm) {
        case IMM_SCAL: ok = imm < lim.n_scal; break;
        case IMM_CONST4: ok = imm >= lim.consts_at && imm + 4 <= lim.n_scal; break;
        case IMM_TAP: ok = imm < lim.n_taps; break;
        case IMM_POW: ok = imm < lim.n_pows; break;
        case IMM_SET: ok = imm < lim.max_set; break;
        case IMM_SUM: ok = imm < lim.sums; break;
        case IMM_PROD: ok = imm >= lim.sums && imm < lim.sequences; break;
        case IMM_DEN: ok = imm >= lim.sequences && imm < (size_t)lim.sequences + lim.ratios; break;
        default: break;  // IMM_NONE
        }
        if (!ok) return false;
    }
    return true;
}

bool program_fits(const bx_cons_program* p) {
    const bx_cons_program_info& in = p->info;
    const size_t at = (size_t)in.n_globals + 4;
    return p->ret_slot < in.wide && p->n_pows >= 1 &&
           stream_fits(p->code, StreamLimits{KIND_CONS, in.narrow, in.wide, at + p->consts.size(), at, p->taps.data(), p->taps.size(), 3, p->n_pows, 0, 0, 0, 0});
}

bool program_fits(const bx_wit_program* p) {  // `scal` is the constants alone
    return stream_fits(p->code, StreamLimits{KIND_WIT, p->info.narrow, 0, p->consts.size(), 0, p->taps.data(), p->taps.size(), 2, 0, p->max_set, 0, 0, 0});
}

bool program_fits(const bx_acc_program* p) {
    const bx_acc_program_info& in = p->info;
    if (in.sequences < 1 || in.sequences > BX_ACC_MAX_SEQS || in.sums > in.sequences || p->ratios > in.sequences - in.sums || p->tap_kept.size() != p->taps.size() ||
        in.kept != p->kept.size())
        return false;
    for (uint32_t k : p->tap_kept)
        if (k >= p->kept.size()) return false;
    for (const bx_cons_tap& t : p->kept)
        if (t.group > 1) return false;
    const size_t at = (size_t)in.n_globals + 4;
    return stream_fits(p->code, StreamLimits{KIND_ACC, in.narrow, in.wide, at + p->consts.size(), at, p->taps.data(), p->taps.size(), 2, 0, 0, in.sums, in.sequences, p->ratios});
}

const char* acc_program_check_widths(const std::vector<bx_cons_tap>& kept, const char* who, uint32_t w_code, uint32_t w_data) {
    for (size_t k = 0; k < kept.size(); ++k) {
        const bx_cons_tap& t = kept[k];
        const uint32_t w = t.group == 0 ? w_code : w_data;
        if (t.col >= w) return refuse("%s: the program taps column %u of group %u (kept column %zu), which has %u columns", who, t.col, t.group, k, w);
    }
    return nullptr;
}

const char* wit_program_check_widths(const uint32_t max_col[2], uint32_t max_set, const char* who, uint32_t w_code, uint32_t w_data) {
    const uint32_t widths[2] = {w_code, w_data};
    for (int g = 0; g < 2; ++g)
        if (max_col[g] > widths[g]) return refuse("%s: the program taps column %u of group %d, which has %u columns", who, max_col[g] - 1, g, widths[g]);
    if (max_set > w_data) return refuse("%s: the program sets data column %u, the data group has %u columns", who, max_set - 1, w_data);
    return nullptr;
}

const char* wit_program_check_counts(const std::vector<WitCount>& counts, const char* who, uint32_t po2, uint32_t w_data) {
    const uint32_t n = 1u << po2;
    for (size_t k = 0; k < counts.size(); ++k) {
        const WitCount& ct = counts[k];
        if (ct.rows > n) return refuse("%s: count %zu: rows %u is above the trace's %u rows", who, k, ct.rows, n);
        if (ct.rows == 0 && ct.bins > n) return refuse("%s: count %zu: bins %u is above the trace's %u rows (rows == 0 counts all of them)", who, k, ct.bins, n);
        if (ct.col >= w_data) return refuse("%s: count %zu fills data column %u, the data group has %u columns", who, k, ct.col, w_data);
        for (size_t q = 0; q < ct.sources.size(); ++q)
            if (ct.sources[q] >= w_data) return refuse("%s: count %zu: source %zu is data column %u, the data group has %u columns", who, k, q, ct.sources[q], w_data);
    }
    return nullptr;
}

const char* wit_program_check_sorts(const std::vector<WitSort>& sorts, const char* who, uint32_t po2, uint32_t w_data) {
    const uint32_t n = 1u << po2;
    for (size_t k = 0; k < sorts.size(); ++k) {
        const WitSort& s = sorts[k];
        if (s.rows > n) return refuse("%s: sort %zu: rows %u is above the trace's %u rows", who, k, s.rows, n);
        for (size_t q = 0; q < s.sources.size(); ++q)
            if (s.sources[q] >= w_data) return refuse("%s: sort %zu: source %zu is data column %u, the data group has %u columns", who, k, q, s.sources[q], w_data);
        for (size_t q = 0; q < s.dests.size(); ++q)
            if (s.dests[q] >= w_data) return refuse("%s: sort %zu: dest %zu is data column %u, the data group has %u columns", who, k, q, s.dests[q], w_data);
    }
    return nullptr;
}

namespace {

// `scal` of a constraint or an accumulate program for one call: [globals | mix (4) | constants]
std::vector<uint32_t> scal_table(uint32_t ng, const uint32_t* globals, const uint32_t mix[4], const std::vector<uint32_t>& consts) {
    std::vector<uint32_t> scal(ng + 4 + consts.size());
    for (uint32_t i = 0; i < ng; ++i) scal[i] = globals[i];
    for (uint32_t i = 0; i < 4; ++i) scal[ng + i] = mix[i];
    std::copy(consts.begin(), consts.end(), scal.begin() + ng + 4);
    return scal;
}

// One instruction for one row, on the prover's types: the host twin of cp_exec (cons_program_exec.hpp), over a narrow file of words and
// a wide file of Fp4, canonical arithmetic in the device's operand order.  The caller has held the stream against program_fits: no
// slot or table index is checked here.  `env` supplies tap(imm), says with Env::EXT whether the kind has ext values at all (without
// them `wid` is never touched), and executes the opcodes this function does not know in other(): CP_ST, the term stores.
template <class Env>
void host_exec(uint32_t w0, uint32_t w1, uint32_t* nar, Fp4* wid, const std::vector<uint32_t>& scal, Env& env) {
    const uint32_t op = w0 & 0xFFu, dst = (w0 >> 8) & 0xFFu, a = (w0 >> 16) & 0xFFu, b = w0 >> 24, imm = w1 >> 8;
    switch (op) {
    case CP_NOP: return;
    case CP_LD_B: nar[dst] = scal[imm]; return;
    case CP_TAP: nar[dst] = env.tap(imm); return;
    case CP_ADD_BB: nar[dst] = fp_add(nar[a], nar[b]); return;
    case CP_SUB_BB: nar[dst] = fp_sub(nar[a], nar[b]); return;
    case CP_MUL_BB: nar[dst] = fp_mul(nar[a], nar[b]); return;
    default: break;
    }
    if (!Env::EXT) return env.other(op, a, b, imm, nar, wid);
    switch (op) {
    case CP_LD_E: wid[dst] = Fp4{{scal[imm], scal[imm + 1], scal[imm + 2], scal[imm + 3]}}; return;
    case CP_ADD_EB: {
        Fp4 x = wid[a];
        x.c[0] = fp_add(x.c[0], nar[b]);
        wid[dst] = x;
        return;
    }
    case CP_SUB_EB: {
        Fp4 x = wid[a];
        x.c[0] = fp_sub(x.c[0], nar[b]);
        wid[dst] = x;
        return;
    }
    case CP_SUB_BE: wid[dst] = Fp4{{fp_sub(nar[a], wid[b].c[0]), fp_neg(wid[b].c[1]), fp_neg(wid[b].c[2]), fp_neg(wid[b].c[3])}}; return;
    case CP_MUL_EB: wid[dst] = f4_scale(wid[a], nar[b]); return;
    case CP_ADD_EE: wid[dst] = f4_add(wid[a], wid[b]); return;
    case CP_SUB_EE: wid[dst] = f4_sub(wid[a], wid[b]); return;
    case CP_MUL_EE: wid[dst] = f4_mul(wid[a], wid[b]); return;
    default: return env.other(op, a, b, imm, nar, wid);
    }
}

// a tap of a row executor: column `col` of `code` or `data` (N words each) at row r - back, cyclic
uint32_t row_tap(const bx_cons_tap& t, const uint32_t* code, const uint32_t* data, size_t n, size_t r) {
    const uint32_t* col = (t.group == 0 ? code : data) + (size_t)t.col * n;
    return col[((uint32_t)r - t.back) & (uint32_t)(n - 1)];  // N divides 2^32: the wrapped difference reduces properly
}

struct WitEnv {
    static constexpr bool EXT = false;
    const bx_wit_program* prog;
    const uint32_t* code;
    uint32_t* data;
    size_t n, r;
    uint32_t tap(uint32_t imm) const { return row_tap(prog->taps[imm], code, data, n, r); }
    void other(uint32_t op, uint32_t a, uint32_t, uint32_t imm, const uint32_t* nar, const Fp4*) const {
        if (op == CP_ST) data[(size_t)imm * n + r] = nar[a];
    }
};

struct AccEnv {
    static constexpr bool EXT = true;
    const bx_acc_program* prog;
    const uint32_t* code;
    const uint32_t* data;
    Fp4* run;         // the device's run_ext: sequence-major AoS
    uint32_t* mults;
    size_t n, r;
    uint32_t tap(uint32_t imm) const { return row_tap(prog->taps[imm], code, data, n, r); }
    void other(uint32_t op, uint32_t a, uint32_t b, uint32_t imm, const uint32_t* nar, const Fp4* wid) const {
        switch (op) {
        case CP_TSUM_B:
        case CP_TSUM_E:
            run[(size_t)imm * n + r] = op == CP_TSUM_B ? Fp4{{nar[b], 0u, 0u, 0u}} : wid[b];
            mults[(size_t)imm * n + r] = nar[a];
            return;
        case CP_TPROD_B:
        case CP_TDEN_B:  // the denominators of the R ratios: sequences [S, S + R) of `run`
            run[(size_t)imm * n + r] = Fp4{{nar[a], 0u, 0u, 0u}};
            return;
        case CP_TPROD_E:
        case CP_TDEN_E:
            run[(size_t)imm * n + r] = wid[a];
            return;
        default: return;
        }
    }
};

}  // namespace
}  // namespace bx

// ---- constraint programs ----
extern "C" void bx_cons_program_destroy(bx_cons_program* prog) { delete prog; }

extern "C" const char* bx_cons_program_info_get(const bx_cons_program* prog, bx_cons_program_info* out) {
    if (!prog || !out) return "bx_cons_program_info_get: null argument";
    *out = prog->info;
    return nullptr;
}

extern "C" uint32_t bx_cons_program_taps(const bx_cons_program* prog, int group, uint32_t col, uint32_t backs_out[BX_MAX_TAPS]) {
    uint32_t n = 0;
    backs_out[n++] = 0;
    if (!prog) return n;
    // at most BX_MAX_TAPS distinct values by construction (create refuses a ninth); insertion keeps them sorted
    for (const bx_cons_tap& t : prog->taps) {
        if ((int)t.group != group || t.col != col) continue;
        uint32_t k = 0;
        while (k < n && backs_out[k] < t.back) ++k;
        if (k < n && backs_out[k] == t.back) continue;
        for (uint32_t j = n; j > k; --j) backs_out[j] = backs_out[j - 1];
        backs_out[k] = t.back;
        ++n;
    }
    return n;
}

// On the verifier every value is ext: the narrow file holds Fp4 too, so this executor shares no instruction body with host_exec.
extern "C" const char* bx_cons_program_constraints_at(const bx_cons_program* prog, const bx_tap_reader* taps, const uint32_t poly_mix[4], const uint32_t mix[4],
                                                      const uint32_t* globals, uint32_t out[4]) try {
    using namespace bx;
    if (!prog || !taps || !taps->at || !poly_mix || !mix || !out) return "bx_cons_program_constraints_at: null argument";
    if (prog->info.n_globals && !globals) return "bx_cons_program_constraints_at: the program names globals and none were given";
    if (!program_fits(prog)) return "bx_cons_program_constraints_at: corrupt instruction stream";  // as long as the walk it guards
    const std::vector<uint32_t> scal = scal_table(prog->info.n_globals, globals, mix, prog->consts);
    std::vector<Fp4> pows(prog->n_pows);
    const Fp4 pm{{poly_mix[0], poly_mix[1], poly_mix[2], poly_mix[3]}};
    pows[0] = f4_one();
    for (uint32_t e = 1; e < prog->n_pows; ++e) pows[e] = f4_mul(pows[e - 1], pm);
    Fp4 nar[BX_CONS_MAX_NARROW], wid[BX_CONS_MAX_WIDE];
    for (Fp4& v : nar) v = f4_zero();
    for (Fp4& v : wid) v = f4_zero();
    const char* err = nullptr;
    const auto base = [](uint32_t w) { return Fp4{{w, 0u, 0u, 0u}}; };
    for (size_t pc = 0; pc < prog->code.size(); pc += 2) {
        const uint32_t w0 = prog->code[pc], w1 = prog->code[pc + 1];
        const uint32_t op = w0 & 0xFFu, dst = (w0 >> 8) & 0xFFu, a = (w0 >> 16) & 0xFFu, b = w0 >> 24, c = w1 & 0xFFu, imm = w1 >> 8;
        switch (op) {
        case CP_LD_B: nar[dst] = base(scal[imm]); break;
        case CP_LD_E: wid[dst] = Fp4{{scal[imm], scal[imm + 1], scal[imm + 2], scal[imm + 3]}}; break;
        case CP_TAP: {
            const bx_cons_tap& t = prog->taps[imm];
            Fp4 v = f4_zero();
            if (const char* e = taps->at(taps->ctx, (int)t.group, t.col, (int)t.back, v.c)) {
                err = e;
                v = f4_zero();
            }
            nar[dst] = v;
            break;
        }
        case CP_ADD_BB: nar[dst] = f4_add(nar[a], nar[b]); break;
        case CP_SUB_BB: nar[dst] = f4_sub(nar[a], nar[b]); break;
        case CP_MUL_BB: nar[dst] = f4_mul(nar[a], nar[b]); break;
        case CP_ADD_EB: wid[dst] = f4_add(wid[a], nar[b]); break;
        case CP_SUB_EB: wid[dst] = f4_sub(wid[a], nar[b]); break;
        case CP_SUB_BE: wid[dst] = f4_sub(nar[a], wid[b]); break;
        case CP_MUL_EB: wid[dst] = f4_mul(wid[a], nar[b]); break;
        case CP_ADD_EE: wid[dst] = f4_add(wid[a], wid[b]); break;
        case CP_SUB_EE: wid[dst] = f4_sub(wid[a], wid[b]); break;
        case CP_MUL_EE: wid[dst] = f4_mul(wid[a], wid[b]); break;
        case CP_ZERO: wid[dst] = f4_zero(); break;
        case CP_EQZ_B: wid[dst] = f4_add(wid[a], f4_mul(pows[imm], nar[b])); break;
        case CP_EQZ_E: wid[dst] = f4_add(wid[a], f4_mul(pows[imm], wid[b])); break;
        case CP_COND_B: wid[dst] = f4_add(wid[a], f4_mul(f4_mul(pows[imm], wid[c]), nar[b])); break;
        case CP_COND_E: wid[dst] = f4_add(wid[a], f4_mul(f4_mul(pows[imm], wid[c]), wid[b])); break;
        default: break;  // CP_NOP, the padding
        }
    }
    memcpy(out, wid[prog->ret_slot].c, 16);
    return err;
} catch (...) {
    return "bx_cons_program_constraints_at: out of host memory";
}

// ---- witness programs ----
extern "C" void bx_wit_program_destroy(bx_wit_program* prog) { delete prog; }

extern "C" const char* bx_wit_program_info_get(const bx_wit_program* prog, bx_wit_program_info* out) {
    if (!prog || !out) return "bx_wit_program_info_get: null argument";
    *out = prog->info;
    return nullptr;
}

extern "C" uint32_t bx_wit_program_counts(const bx_wit_program* prog) { return prog ? (uint32_t)prog->counts.size() : 0u; }

extern "C" const char* bx_wit_program_count_get(const bx_wit_program* prog, uint32_t i, uint32_t* col, uint32_t* bins, uint32_t* rows, uint32_t* sources_out,
                                                uint32_t cap, uint32_t* n_sources) {
    if (!prog || !col || !bins || !rows || !n_sources || (cap && !sources_out)) return "bx_wit_program_count_get: null argument";
    if (i >= prog->counts.size()) return "bx_wit_program_count_get: index is not below the number of counts";
    const bx::WitCount& ct = prog->counts[i];
    *col = ct.col, *bins = ct.bins, *rows = ct.rows;
    *n_sources = (uint32_t)ct.sources.size();
    for (uint32_t q = 0; q < cap && q < ct.sources.size(); ++q) sources_out[q] = ct.sources[q];
    return nullptr;
}

extern "C" uint32_t bx_wit_program_sorts(const bx_wit_program* prog) { return prog ? (uint32_t)prog->sorts.size() : 0u; }

extern "C" const char* bx_wit_program_sort_get(const bx_wit_program* prog, uint32_t i, uint32_t* rows, uint32_t* n_keys, uint32_t bits_out[BX_WIT_MAX_SORT_KEYS],
                                               uint32_t* sources_out, uint32_t* dests_out, uint32_t cap, uint32_t* n_cols) {
    if (!prog || !rows || !n_keys || !bits_out || !n_cols || (cap && (!sources_out || !dests_out))) return "bx_wit_program_sort_get: null argument";
    if (i >= prog->sorts.size()) return "bx_wit_program_sort_get: index is not below the number of sorts";
    const bx::WitSort& s = prog->sorts[i];
    *rows = s.rows;
    *n_keys = (uint32_t)s.bits.size();
    *n_cols = (uint32_t)s.sources.size();
    for (size_t q = 0; q < s.bits.size() && q < BX_WIT_MAX_SORT_KEYS; ++q) bits_out[q] = s.bits[q];
    for (uint32_t q = 0; q < cap && q < s.sources.size(); ++q) sources_out[q] = s.sources[q], dests_out[q] = s.dests[q];
    return nullptr;
}

extern "C" int bx_wit_program_derives(const bx_wit_program* prog, uint32_t col) {
    if (!prog) return 0;
    if (std::find(prog->sets.begin(), prog->sets.end(), col) != prog->sets.end()) return 1;
    for (const bx::WitCount& ct : prog->counts)
        if (ct.col == col) return 1;
    for (const bx::WitSort& s : prog->sorts)
        if (std::find(s.dests.begin(), s.dests.end(), col) != s.dests.end()) return 1;
    return 0;
}

extern "C" const char* bx_wit_program_run_host(const bx_wit_program* prog, uint32_t po2, const uint32_t* code, uint32_t w_code, uint32_t* data, uint32_t w_data) try {
    using namespace bx;
    if (!prog || (w_code && !code) || (w_data && !data)) return "bx_wit_program_run_host: null argument";
    if (po2 < 1 || po2 > 24) return "bx_wit_program_run_host: po2 must be in [1, 24]";
    if (const char* e = wit_program_check_widths(prog->max_col, prog->max_set, "bx_wit_program_run_host", w_code, w_data)) return e;
    if (const char* e = wit_program_check_sorts(prog->sorts, "bx_wit_program_run_host", po2, w_data)) return e;
    if (const char* e = wit_program_check_counts(prog->counts, "bx_wit_program_run_host", po2, w_data)) return e;
    if (!program_fits(prog)) return "bx_wit_program_run_host: corrupt instruction stream";
    const size_t n = (size_t)1 << po2;
    // rows in any order: no row reads a word this run writes (derived cells are forwarded, never loaded)
    for (size_t r = 0; r < n; ++r) {
        uint32_t nar[BX_CONS_MAX_NARROW] = {};
        WitEnv env{prog, code, data, n, r};
        for (size_t pc = 0; pc < prog->code.size(); pc += 2) host_exec(prog->code[pc], prog->code[pc + 1], nar, nullptr, prog->consts, env);
    }
    // the sorts, in list order, after every row and before the counts: pi = the stable sort of rows [0, rows) by the decoded, masked key
    // tuple; every source gathered into a temporary before a dest is written
    for (const WitSort& s : prog->sorts) {
        const size_t rows = s.rows ? s.rows : n, nk = s.bits.size();
        std::vector<uint32_t> keys(rows * nk), pi(rows);
        for (size_t k = 0; k < nk; ++k) {
            const uint32_t mask = (uint32_t)(((uint64_t)1 << s.bits[k]) - 1);
            for (size_t r = 0; r < rows; ++r) keys[r * nk + k] = fp_decode(data[(size_t)s.sources[k] * n + r]) & mask;
        }
        for (size_t r = 0; r < rows; ++r) pi[r] = (uint32_t)r;
        std::stable_sort(pi.begin(), pi.end(), [&](uint32_t a, uint32_t b) {
            return std::lexicographical_compare(&keys[a * nk], &keys[a * nk] + nk, &keys[b * nk], &keys[b * nk] + nk);
        });
        std::vector<uint32_t> tmp(rows * s.sources.size());
        for (size_t q = 0; q < s.sources.size(); ++q)
            for (size_t r = 0; r < rows; ++r) tmp[q * rows + r] = data[(size_t)s.sources[q] * n + pi[r]];
        for (size_t q = 0; q < s.dests.size(); ++q)
            for (size_t r = 0; r < rows; ++r) data[(size_t)s.dests[q] * n + r] = tmp[q * rows + r];
    }
    // the counts, in list order, after the sorts: the device path's twin (clear, histogram over rows [0, rows), store)
    for (const WitCount& ct : prog->counts) {
        const size_t rows = ct.rows ? ct.rows : n;
        std::vector<uint32_t> bins(ct.bins, 0u);
        for (uint32_t src : ct.sources)
            for (size_t j = 0; j < rows; ++j) {
                const uint32_t v = fp_decode(data[(size_t)src * n + j]);
                if (v < ct.bins) ++bins[v];  // at most 64 * 2^24 = 2^30 < P: no wrap, no reduction
            }
        for (size_t r = 0; r < rows; ++r) data[(size_t)ct.col * n + r] = r < ct.bins ? fp_mul(R2, bins[r]) : 0u;
    }
    return nullptr;
} catch (...) {
    return "bx_wit_program_run_host: out of host memory";
}

// ---- accumulate programs ----
extern "C" void bx_acc_program_destroy(bx_acc_program* prog) { delete prog; }

extern "C" const char* bx_acc_program_info_get(const bx_acc_program* prog, bx_acc_program_info* out) {
    if (!prog || !out) return "bx_acc_program_info_get: null argument";
    *out = prog->info;
    return nullptr;
}

extern "C" const char* bx_acc_program_kept(const bx_acc_program* prog, uint32_t i, uint32_t* group, uint32_t* col) {
    if (!prog || !group || !col) return "bx_acc_program_kept: null argument";
    if (i >= prog->kept.size()) return "bx_acc_program_kept: index is not below the number of kept columns";
    *group = prog->kept[i].group;
    *col = prog->kept[i].col;
    return nullptr;
}

extern "C" const char* bx_acc_program_ratios(const bx_acc_program* prog, uint32_t* out) {
    if (!prog || !out) return "bx_acc_program_ratios: null argument";
    *out = prog->ratios;
    return nullptr;
}

extern "C" const char* bx_acc_program_run_host(const bx_acc_program* prog, uint32_t po2, const uint32_t* code, uint32_t w_code, const uint32_t* data,
                                               uint32_t w_data, const uint32_t* globals, const uint32_t mix[4], uint32_t* accum, uint32_t w_accum) try {
    using namespace bx;
    if (!prog || !mix || !accum || (w_code && !code) || (w_data && !data)) return "bx_acc_program_run_host: null argument";
    if (prog->info.n_globals && !globals) return "bx_acc_program_run_host: the program names globals and none were given";
    if (po2 < 1 || po2 > 24) return "bx_acc_program_run_host: po2 must be in [1, 24]";
    if (const char* e = acc_program_check_widths(prog->kept, "bx_acc_program_run_host", w_code, w_data)) return e;
    const uint32_t S = prog->info.sequences, sums = prog->info.sums;
    if (w_accum < 4 * S) return refuse("bx_acc_program_run_host: the program writes %u accum columns, the accum group has %u", 4 * S, w_accum);
    if (!program_fits(prog)) return "bx_acc_program_run_host: corrupt instruction stream";
    const size_t n = (size_t)1 << po2;
    const std::vector<uint32_t> scal = scal_table(prog->info.n_globals, globals, mix, prog->consts);
    const uint32_t R = prog->ratios;
    std::vector<Fp4> run((size_t)(S + R) * n, f4_zero());
    std::vector<uint32_t> mults((size_t)sums * n, 0u);
    // (1) the terms of every row
    for (size_t r = 0; r < n; ++r) {
        uint32_t nar[BX_CONS_MAX_NARROW] = {};
        Fp4 wid[BX_CONS_MAX_WIDE];
        for (Fp4& v : wid) v = f4_zero();
        AccEnv env{prog, code, data, run.data(), mults.data(), n, r};
        for (size_t pc = 0; pc < prog->code.size(); pc += 2) host_exec(prog->code[pc], prog->code[pc + 1], nar, wid, scal, env);
    }
    // (2) m / d with 0 -> 0 and the running sums; (3) a / b with 1 / 0 -> 0 for the ratios, and the running products; (4) sequence s,
    // component k -> column 4 s + k
    for (uint32_t s = 0; s < S; ++s) {
        Fp4 acc = s < sums ? f4_zero() : f4_one();
        for (size_t r = 0; r < n; ++r) {
            const Fp4& v = run[(size_t)s * n + r];
            if (s < sums) acc = f4_add(acc, f4_is_zero(v) ? f4_zero() : f4_scale(f4_inv(v), mults[(size_t)s * n + r]));
            else if (s >= S - R) {
                const Fp4& d = run[(size_t)(s + R) * n + r];
                acc = f4_mul(acc, f4_is_zero(d) ? f4_zero() : f4_mul(v, f4_inv(d)));
            }
            else acc = f4_mul(acc, v);
            for (uint32_t k = 0; k < 4; ++k) accum[(size_t)(4 * s + k) * n + r] = acc.c[k];
        }
    }
    return nullptr;
} catch (...) {
    return "bx_acc_program_run_host: out of host memory";
}
