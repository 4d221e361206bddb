// cons_program_host.cpp — host half of constraint programs (include/bx_program.h is the normative text): the compiler from a step list
// to the instruction stream of cons_program.hpp, and the host executor of that stream over Fp4 (the verifier's constraints_at); and
// the same two for witness programs, which share the slot allocation and the instruction format (compile_wit, bx_wit_program_run_host),
// and for accumulate programs (compile_acc, bx_acc_program_run_host).
// No HIP: this translation unit compiles with plain g++ (tests/cons_program_check.cpp runs it under sanitizers).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <new>
#include <set>
#include <utility>

#include "cons_program.hpp"
#include "fp.hpp"

namespace bx {
namespace {

thread_local char g_msg[512];
const char* refuse(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return g_msg;
}

constexpr uint32_t NEVER = 0xFFFFFFFFu;

struct FpVar {
    bool ext = false;
    uint32_t degree = 0, slot = 0, last_use = 0;  // last_use: the step that reads it last (its own step if none does)
};
struct MixVar {
    uint32_t exp = 0, degree = 0, slot = 0, last_use = 0;
};

// a bounded slot file: the lowest free slot first, so that a program's footprint is its peak of live values
struct SlotFile {
    std::set<uint32_t> free_;
    uint32_t top = 0, live = 0, peak = 0;
    uint32_t take() {
        ++live;
        peak = std::max(peak, live);
        if (!free_.empty()) {
            const uint32_t s = *free_.begin();
            free_.erase(free_.begin());
            return s;
        }
        return top++;
    }
    void give(uint32_t s) {
        --live;
        free_.insert(s);
    }
};

const char* compile(const bx_cons_program_desc* d, bx_cons_program* p) {
    if (d->n_steps > BX_CONS_MAX_STEPS) return refuse("cons_program: %zu steps, more than BX_CONS_MAX_STEPS = %d", d->n_steps, BX_CONS_MAX_STEPS);
    if (d->n_taps > BX_CONS_MAX_TAPS) return refuse("cons_program: %zu taps, more than BX_CONS_MAX_TAPS = %d", d->n_taps, BX_CONS_MAX_TAPS);
    if (d->n_globals > BX_MAX_GLOBALS) return refuse("cons_program: n_globals %u is above BX_MAX_GLOBALS = %d", d->n_globals, BX_MAX_GLOBALS);
    if ((d->n_steps && !d->steps) || (d->n_taps && !d->taps)) return refuse("cons_program: null step or tap list");

    // ---- the tap list: ranges, and the tap set of every named column ----
    std::map<std::pair<uint32_t, uint32_t>, std::set<uint32_t>> sets;
    for (size_t t = 0; t < d->n_taps; ++t) {
        const bx_cons_tap& tp = d->taps[t];
        if (tp.group > 2) return refuse("cons_program: tap %zu: tap group %u out of range (0 code, 1 data, 2 accum)", t, tp.group);
        if (tp.col > BX_CONS_MAX_COL) return refuse("cons_program: tap %zu: tap column %u out of range (at most %d)", t, tp.col, BX_CONS_MAX_COL);
        if (tp.back > BX_CONS_MAX_BACK) return refuse("cons_program: tap %zu: tap back %u out of range (at most %d)", t, tp.back, BX_CONS_MAX_BACK);
        std::set<uint32_t>& s = sets[{tp.group, tp.col}];
        s.insert(0u);
        s.insert(tp.back);
        if (s.size() > BX_MAX_TAPS)
            return refuse("cons_program: tap %zu: more than BX_MAX_TAPS = %d distinct backs on column %u of group %u", t, BX_MAX_TAPS, tp.col, tp.group);
        p->max_col[tp.group] = std::max(p->max_col[tp.group], tp.col + 1);
    }
    p->taps.assign(d->taps, d->taps + d->n_taps);

    // ---- pass 1: validation, types, mix exponents, degrees, last uses ----
    std::vector<FpVar> fp;
    std::vector<MixVar> mix;
    std::vector<uint32_t> var_of(d->n_steps);  // step -> its var's index in its list
    const auto use_fp = [&](size_t i, const char* what, uint32_t v) -> const char* {
        if (v >= fp.size()) return refuse("cons_program: step %zu: operand %s = %u refers to a later or missing fp var (%zu so far)", i, what, v, fp.size());
        fp[v].last_use = (uint32_t)i;
        return nullptr;
    };
    const auto use_mix = [&](size_t i, const char* what, uint32_t v) -> const char* {
        if (v >= mix.size()) return refuse("cons_program: step %zu: operand %s = %u refers to a later or missing mix var (%zu so far)", i, what, v, mix.size());
        mix[v].last_use = (uint32_t)i;
        return nullptr;
    };
#define CP_TRY(expr)                 \
    do {                             \
        const char* _m = (expr);     \
        if (_m) return _m;           \
    } while (0)
    for (size_t i = 0; i < d->n_steps; ++i) {
        const bx_cons_step& s = d->steps[i];
        FpVar f;
        MixVar m;
        f.last_use = m.last_use = (uint32_t)i;
        bool is_mix = false;
        switch (s.op) {
        case BX_CONS_CONST:
            if (s.a >= P) return refuse("cons_program: step %zu: constant %u is not below P", i, s.a);
            break;
        case BX_CONS_CONST_EXT:
            if (s.a >= P || s.b >= P || s.c >= P || s.d >= P) return refuse("cons_program: step %zu: ext constant (%u, %u, %u, %u) has a component not below P", i, s.a, s.b, s.c, s.d);
            f.ext = true;
            break;
        case BX_CONS_GET:
            if (s.a >= d->n_taps) return refuse("cons_program: step %zu: tap index %u out of range (%zu taps)", i, s.a, d->n_taps);
            f.degree = 1;
            break;
        case BX_CONS_GET_GLOBAL:
            if (s.a > 1) return refuse("cons_program: step %zu: GET_GLOBAL table %u out of range (0 globals, 1 mix)", i, s.a);
            if (s.a == 0 && s.b >= d->n_globals) return refuse("cons_program: step %zu: global index %u out of range (%u globals)", i, s.b, d->n_globals);
            if (s.a == 1 && s.b >= 4) return refuse("cons_program: step %zu: mix component %u out of range (an ext element has 4)", i, s.b);
            break;
        case BX_CONS_ADD:
        case BX_CONS_SUB:
        case BX_CONS_MUL:
            CP_TRY(use_fp(i, "a", s.a));
            CP_TRY(use_fp(i, "b", s.b));
            f.ext = fp[s.a].ext || fp[s.b].ext;
            f.degree = s.op == BX_CONS_MUL ? fp[s.a].degree + fp[s.b].degree : std::max(fp[s.a].degree, fp[s.b].degree);
            break;
        case BX_CONS_TRUE:
            is_mix = true;
            break;
        case BX_CONS_AND_EQZ:
            is_mix = true;
            CP_TRY(use_mix(i, "a", s.a));
            CP_TRY(use_fp(i, "b", s.b));
            m.exp = mix[s.a].exp + 1;
            m.degree = std::max(mix[s.a].degree, fp[s.b].degree);
            break;
        case BX_CONS_AND_COND:
            is_mix = true;
            CP_TRY(use_mix(i, "a", s.a));
            CP_TRY(use_fp(i, "b", s.b));
            CP_TRY(use_mix(i, "c", s.c));
            m.exp = mix[s.a].exp + mix[s.c].exp;
            m.degree = std::max(mix[s.a].degree, fp[s.b].degree + mix[s.c].degree);
            break;
        default:
            return refuse("cons_program: step %zu: unknown op %u", i, s.op);
        }
        const uint32_t deg = is_mix ? m.degree : f.degree;
        if (deg > BX_CONS_MAX_DEGREE)
            return refuse("cons_program: step %zu: degree %u is above BX_CONS_MAX_DEGREE = %d (the quotient would not fit the 4N check evaluations)", i, deg, BX_CONS_MAX_DEGREE);
        if (is_mix && m.exp > BX_CONS_MAX_STEPS) return refuse("cons_program: step %zu: %u constraints, more than BX_CONS_MAX_STEPS = %d", i, m.exp, BX_CONS_MAX_STEPS);
        if (is_mix) {
            var_of[i] = (uint32_t)mix.size();
            mix.push_back(m);
        } else {
            var_of[i] = (uint32_t)fp.size();
            fp.push_back(f);
        }
    }
    if (d->ret >= mix.size()) return refuse("cons_program: ret = %u is not a mix var (%zu mix vars)", d->ret, mix.size());
    mix[d->ret].last_use = NEVER;

    // ---- pass 2: slots by last use, and the stream ----
    SlotFile narrow, wide;
    const uint32_t scal_consts = d->n_globals + 4;  // where the constants start in `scal`
    uint32_t n_pows = 1;
    const auto emit = [&](uint32_t op, uint32_t dst, uint32_t a, uint32_t b, uint32_t c, uint32_t imm) {
        p->code.push_back(cp_w0(op, dst, a, b));
        p->code.push_back(cp_w1(c, imm));
    };
    uint32_t fi = 0, mi = 0;
    for (size_t i = 0; i < d->n_steps; ++i) {
        const bx_cons_step& s = d->steps[i];
        const uint32_t step = (uint32_t)i;
        // operands that die here give their slots back BEFORE the result takes one (dst may alias a source: executors read first)
        const auto drop_fp = [&](uint32_t v) {
            if (fp[v].last_use == step) {
                (fp[v].ext ? wide : narrow).give(fp[v].slot);
                fp[v].last_use = NEVER - 1;  // an operand named twice is dropped once
            }
        };
        const auto drop_mix = [&](uint32_t v) {
            if (mix[v].last_use == step) {
                wide.give(mix[v].slot);
                mix[v].last_use = NEVER - 1;
            }
        };
        const bool is_mix = s.op >= BX_CONS_TRUE;
        uint32_t dst = 0;
        if (!is_mix) {
            FpVar& f = fp[fi];
            const bool unused = f.last_use == step;
            uint32_t sa = 0, sb = 0;
            bool ea = false, eb = false;
            if (s.op >= BX_CONS_ADD) {
                sa = fp[s.a].slot, sb = fp[s.b].slot, ea = fp[s.a].ext, eb = fp[s.b].ext;
                drop_fp(s.a);
                drop_fp(s.b);
            }
            dst = f.slot = (f.ext ? wide : narrow).take();
            switch (s.op) {
            case BX_CONS_CONST:
                emit(CP_LD_B, dst, 0, 0, 0, scal_consts + (uint32_t)p->consts.size());
                p->consts.push_back(fp_encode(s.a));
                break;
            case BX_CONS_CONST_EXT:
                emit(CP_LD_E, dst, 0, 0, 0, scal_consts + (uint32_t)p->consts.size());
                for (uint32_t v : {s.a, s.b, s.c, s.d}) p->consts.push_back(fp_encode(v));
                break;
            case BX_CONS_GET:
                emit(CP_TAP, dst, 0, 0, 0, s.a);
                break;
            case BX_CONS_GET_GLOBAL:
                emit(CP_LD_B, dst, 0, 0, 0, s.a == 0 ? s.b : d->n_globals + s.b);
                break;
            case BX_CONS_ADD:
            case BX_CONS_MUL:
                if (!ea && !eb) emit(s.op == BX_CONS_ADD ? CP_ADD_BB : CP_MUL_BB, dst, sa, sb, 0, 0);
                else if (ea && eb) emit(s.op == BX_CONS_ADD ? CP_ADD_EE : CP_MUL_EE, dst, sa, sb, 0, 0);
                else emit(s.op == BX_CONS_ADD ? CP_ADD_EB : CP_MUL_EB, dst, ea ? sa : sb, ea ? sb : sa, 0, 0);  // commutative: ext first
                break;
            default:  // BX_CONS_SUB
                emit(!ea && !eb ? CP_SUB_BB : (ea && eb ? CP_SUB_EE : (ea ? CP_SUB_EB : CP_SUB_BE)), dst, sa, sb, 0, 0);
                break;
            }
            if (unused) (f.ext ? wide : narrow).give(dst);
            ++fi;
        } else {
            MixVar& m = mix[mi];
            const bool unused = m.last_use == step;
            if (s.op == BX_CONS_TRUE) {
                dst = m.slot = wide.take();
                emit(CP_ZERO, dst, 0, 0, 0, 0);
            } else {
                const uint32_t sx = mix[s.a].slot, sy = fp[s.b].slot, e = mix[s.a].exp;
                const bool ey = fp[s.b].ext;
                const uint32_t sc = s.op == BX_CONS_AND_COND ? mix[s.c].slot : 0u;
                drop_mix(s.a);
                drop_fp(s.b);
                if (s.op == BX_CONS_AND_COND) drop_mix(s.c);
                dst = m.slot = wide.take();
                if (s.op == BX_CONS_AND_EQZ) emit(ey ? CP_EQZ_E : CP_EQZ_B, dst, sx, sy, 0, e);
                else emit(ey ? CP_COND_E : CP_COND_B, dst, sx, sy, sc, e);
                n_pows = std::max(n_pows, e + 1);
            }
            if (unused) wide.give(dst);
            ++mi;
        }
        if (narrow.peak > BX_CONS_MAX_NARROW || wide.peak > BX_CONS_MAX_WIDE) {
            const bool nw = narrow.peak > BX_CONS_MAX_NARROW;
            return refuse("cons_program: step %zu: the program needs %u live %s values, the limit is %d (BX_CONS_MAX_%s)", i, nw ? narrow.peak : wide.peak,
                          nw ? "narrow (base)" : "wide (ext and mix)", nw ? BX_CONS_MAX_NARROW : BX_CONS_MAX_WIDE, nw ? "NARROW" : "WIDE");
        }
    }
#undef CP_TRY
    p->info.steps = (uint32_t)d->n_steps;
    p->info.constraints = mix[d->ret].exp;
    p->info.degree = mix[d->ret].degree;
    p->info.narrow = narrow.top;
    p->info.wide = wide.top;
    p->info.instructions = (uint32_t)(p->code.size() / 2);
    p->info.taps = (uint32_t)d->n_taps;
    p->info.n_globals = d->n_globals;
    p->n_pows = n_pows;
    p->ret_slot = mix[d->ret].slot;
    while ((p->code.size() / 2) % CP_FETCH) emit(CP_NOP, 0, 0, 0, 0, 0);
    return nullptr;
}


// ---- witness programs ("Witness programs" of bx_program.h): the same slot allocation and instruction format, one list of vars ----
// An fp var is a value in a narrow slot, or — a GET of a derived column after its SET — another name of the var that was stored.
struct WitVar {
    uint32_t root = 0;  // the var that holds the value (itself unless forwarded)
    uint32_t slot = 0, last_use = 0;
};

const char* compile_wit(const bx_wit_program_desc* d, const bx_wit_count* counts, size_t n_counts, bx_wit_program* p) {
    if (d->n_steps > BX_CONS_MAX_STEPS) return refuse("wit_program: %zu steps, more than BX_CONS_MAX_STEPS = %d", d->n_steps, BX_CONS_MAX_STEPS);
    if (d->n_taps > BX_CONS_MAX_TAPS) return refuse("wit_program: %zu taps, more than BX_CONS_MAX_TAPS = %d", d->n_taps, BX_CONS_MAX_TAPS);
    if (d->n_cells > BX_MAX_GLOBALS) return refuse("wit_program: %zu global cells, more than BX_MAX_GLOBALS = %d", d->n_cells, BX_MAX_GLOBALS);
    if ((d->n_steps && !d->steps) || (d->n_taps && !d->taps) || (d->n_cells && !d->cells)) return refuse("wit_program: null step, tap or cell list");

    for (size_t t = 0; t < d->n_taps; ++t) {
        const bx_cons_tap& tp = d->taps[t];
        if (tp.group == 2) return refuse("wit_program: tap %zu: tap group 2 (accum) does not exist when the witness is generated", t);
        if (tp.group > 2) return refuse("wit_program: tap %zu: tap group %u out of range (0 code, 1 data)", t, tp.group);
        if (tp.col > BX_CONS_MAX_COL) return refuse("wit_program: tap %zu: tap column %u out of range (at most %d)", t, tp.col, BX_CONS_MAX_COL);
        if (tp.back > BX_CONS_MAX_BACK) return refuse("wit_program: tap %zu: tap back %u out of range (at most %d)", t, tp.back, BX_CONS_MAX_BACK);
        p->max_col[tp.group] = std::max(p->max_col[tp.group], tp.col + 1);
    }
    p->taps.assign(d->taps, d->taps + d->n_taps);
    std::set<uint32_t> named;
    for (size_t k = 0; k < d->n_cells; ++k) {
        const bx_wit_global_cell& g = d->cells[k];
        if (g.global >= BX_MAX_GLOBALS) return refuse("wit_program: cell %zu: global index %u is not below BX_MAX_GLOBALS = %d", k, g.global, BX_MAX_GLOBALS);
        if (g.col > BX_CONS_MAX_COL) return refuse("wit_program: cell %zu: data column %u out of range (at most %d)", k, g.col, BX_CONS_MAX_COL);
        if (!named.insert(g.global).second) return refuse("wit_program: cell %zu: global index %u is named twice", k, g.global);
    }
    p->cells.assign(d->cells, d->cells + d->n_cells);

    // ---- pass 0: which data columns are derived, and where ----
    std::map<uint32_t, size_t> set_at;  // data column -> the step that SETs it
    for (size_t i = 0; i < d->n_steps; ++i) {
        const bx_cons_step& s = d->steps[i];
        if (s.op != BX_CONS_SET) continue;
        if (s.a > BX_CONS_MAX_COL) return refuse("wit_program: step %zu: SET column %u out of range (at most %d)", i, s.a, BX_CONS_MAX_COL);
        const auto ins = set_at.emplace(s.a, i);
        if (!ins.second) return refuse("wit_program: step %zu: data column %u is SET a second time (first at step %zu)", i, s.a, ins.first->second);
        p->sets.push_back(s.a);
        p->max_set = std::max(p->max_set, s.a + 1);
    }

    // ---- pass 1: validation, forwarding, last uses ----
    std::vector<WitVar> fp;
    const auto use_fp = [&](size_t i, const char* what, uint32_t v) -> const char* {
        if (v >= fp.size()) return refuse("wit_program: step %zu: operand %s = %u refers to a later or missing fp var (%zu so far)", i, what, v, fp.size());
        fp[fp[v].root].last_use = (uint32_t)i;
        return nullptr;
    };
    static const char* const kForbidden[] = {nullptr, "CONST_EXT", nullptr, "GET_GLOBAL", nullptr, nullptr, nullptr, "TRUE", "AND_EQZ", "AND_COND"};
    for (size_t i = 0; i < d->n_steps; ++i) {
        const bx_cons_step& s = d->steps[i];
        WitVar f;
        f.root = (uint32_t)fp.size();
        f.last_use = (uint32_t)i;
        switch (s.op) {
        case BX_CONS_CONST:
            if (s.a >= P) return refuse("wit_program: step %zu: constant %u is not below P", i, s.a);
            break;
        case BX_CONS_GET: {
            if (s.a >= d->n_taps) return refuse("wit_program: step %zu: tap index %u out of range (%zu taps)", i, s.a, d->n_taps);
            const bx_cons_tap& tp = d->taps[s.a];
            const auto it = tp.group == 1 ? set_at.find(tp.col) : set_at.end();
            if (it == set_at.end()) break;  // a free cell: a memory read
            if (tp.back > 0)
                return refuse("wit_program: step %zu: GET of derived data column %u with back %u: another row's value may not have been written yet", i, tp.col, tp.back);
            if (it->second > i) return refuse("wit_program: step %zu: GET of derived data column %u before its SET at step %zu", i, tp.col, it->second);
            f.root = fp[d->steps[it->second].b].root;  // forwarded: the var that was stored (its SET has been validated: it is earlier)
            fp[f.root].last_use = (uint32_t)i;
            break;
        }
        case BX_CONS_ADD:
        case BX_CONS_SUB:
        case BX_CONS_MUL:
            if (const char* m = use_fp(i, "a", s.a)) return m;
            if (const char* m = use_fp(i, "b", s.b)) return m;
            break;
        case BX_CONS_SET:
            if (const char* m = use_fp(i, "b", s.b)) return m;
            continue;  // appends nothing
        default:
            if (s.op < sizeof kForbidden / sizeof kForbidden[0] && kForbidden[s.op])
                return refuse("wit_program: step %zu: %s does not belong in a witness program (CONST, GET, ADD, SUB, MUL, SET)", i, kForbidden[s.op]);
            return refuse("wit_program: step %zu: unknown op %u", i, s.op);
        }
        fp.push_back(f);
    }

    // ---- the count list ("multiplicity columns"): every rule but the shape-dependent ones (wit_program_check_counts); after the step list,
    // so that a description with a bad step is refused for that step as before ----
    if (n_counts > BX_WIT_MAX_COUNTS) return refuse("wit_program: %zu counts, more than BX_WIT_MAX_COUNTS = %d", n_counts, BX_WIT_MAX_COUNTS);
    if (n_counts && !counts) return refuse("wit_program: null count list");
    std::map<uint32_t, size_t> count_of, source_of;  // data column -> the first count that fills it / reads it
    for (size_t k = 0; k < n_counts; ++k) {
        const bx_wit_count& ct = counts[k];
        if (ct.col > BX_CONS_MAX_COL) return refuse("wit_program: count %zu: data column %u out of range (at most %d)", k, ct.col, BX_CONS_MAX_COL);
        if (ct.n_sources == 0) return refuse("wit_program: count %zu: no sources", k);
        if (ct.n_sources > BX_WIT_MAX_COUNT_SOURCES)
            return refuse("wit_program: count %zu: %u sources, more than BX_WIT_MAX_COUNT_SOURCES = %d", k, ct.n_sources, BX_WIT_MAX_COUNT_SOURCES);
        if (!ct.sources) return refuse("wit_program: count %zu: null source list", k);
        if (ct.bins == 0) return refuse("wit_program: count %zu: bins is 0", k);
        if (ct.bins > BX_WIT_MAX_COUNT_BINS) return refuse("wit_program: count %zu: bins %u is above BX_WIT_MAX_COUNT_BINS = %u", k, ct.bins, BX_WIT_MAX_COUNT_BINS);
        if (ct.rows > (1u << 24)) return refuse("wit_program: count %zu: rows %u is above 2^24, the largest trace", k, ct.rows);
        if (ct.rows != 0 && ct.bins > ct.rows) return refuse("wit_program: count %zu: bins %u is above rows %u", k, ct.bins, ct.rows);
        WitCount wc;
        wc.col = ct.col, wc.bins = ct.bins, wc.rows = ct.rows;
        for (uint32_t q = 0; q < ct.n_sources; ++q) {
            const uint32_t src = ct.sources[q];
            if (src > BX_CONS_MAX_COL) return refuse("wit_program: count %zu: source %u: data column %u out of range (at most %d)", k, q, src, BX_CONS_MAX_COL);
            if (std::find(wc.sources.begin(), wc.sources.end(), src) != wc.sources.end())
                return refuse("wit_program: count %zu: source column %u is named twice", k, src);
            wc.sources.push_back(src);
            source_of.emplace(src, k);
        }
        const auto ins = count_of.emplace(ct.col, k);
        if (!ins.second) return refuse("wit_program: count %zu: data column %u is already the column of count %zu", k, ct.col, ins.first->second);
        const auto st = set_at.find(ct.col);
        if (st != set_at.end()) return refuse("wit_program: count %zu: data column %u is also SET (step %zu)", k, ct.col, st->second);
        p->counts.push_back(std::move(wc));
    }
    for (size_t k = 0; k < p->counts.size(); ++k) {  // in list order: the first count whose column is a source is the one named
        const auto src = source_of.find(p->counts[k].col);
        if (src != source_of.end()) return refuse("wit_program: count %zu: data column %u is a source of count %zu", k, p->counts[k].col, src->second);
    }
    if (!count_of.empty())
        for (size_t i = 0; i < d->n_steps; ++i) {
            const bx_cons_step& s = d->steps[i];
            if (s.op != BX_CONS_GET || s.a >= d->n_taps || d->taps[s.a].group != 1) continue;
            const auto it = count_of.find(d->taps[s.a].col);
            if (it != count_of.end())
                return refuse("wit_program: count %zu: data column %u is read by the GET of step %zu: a multiplicity does not exist while the program runs", it->second,
                              it->first, i);
        }

    // ---- pass 2: slots by last use, and the stream ----
    SlotFile narrow;
    const auto emit = [&](uint32_t op, uint32_t dst, uint32_t a, uint32_t b, uint32_t imm) {
        p->code.push_back(cp_w0(op, dst, a, b));
        p->code.push_back(cp_w1(0, imm));
    };
    uint32_t fi = 0;
    for (size_t i = 0; i < d->n_steps; ++i) {
        const bx_cons_step& s = d->steps[i];
        const uint32_t step = (uint32_t)i;
        // an operand that dies here gives its slot back BEFORE the result takes one (dst may alias a source: executors read first)
        const auto drop = [&](uint32_t v) {
            WitVar& r = fp[fp[v].root];
            if (r.last_use == step) {
                narrow.give(r.slot);
                r.last_use = NEVER - 1;  // an operand named twice is dropped once
            }
        };
        if (s.op == BX_CONS_SET) {
            emit(CP_ST, 0, fp[fp[s.b].root].slot, 0, s.a);
            drop(s.b);
            continue;
        }
        WitVar& f = fp[fi];
        if (f.root != fi) {  // a forwarded GET compiles to nothing
            drop(fi);  // ... and one that nothing reads afterwards ends the stored value's life
            ++fi;
            continue;
        }
        const bool unused = f.last_use == step;
        uint32_t sa = 0, sb = 0;
        if (s.op >= BX_CONS_ADD) {
            sa = fp[fp[s.a].root].slot, sb = fp[fp[s.b].root].slot;
            drop(s.a);
            drop(s.b);
        }
        const uint32_t dst = f.slot = narrow.take();
        switch (s.op) {
        case BX_CONS_CONST:
            emit(CP_LD_B, dst, 0, 0, (uint32_t)p->consts.size());
            p->consts.push_back(fp_encode(s.a));
            break;
        case BX_CONS_GET: emit(CP_TAP, dst, 0, 0, s.a); break;
        case BX_CONS_ADD: emit(CP_ADD_BB, dst, sa, sb, 0); break;
        case BX_CONS_SUB: emit(CP_SUB_BB, dst, sa, sb, 0); break;
        default: emit(CP_MUL_BB, dst, sa, sb, 0); break;
        }
        if (unused) narrow.give(dst);
        ++fi;
        if (narrow.peak > BX_CONS_MAX_NARROW)
            return refuse("wit_program: step %zu: the program needs %u live values, the limit is %d (BX_CONS_MAX_NARROW)", i, narrow.peak, BX_CONS_MAX_NARROW);
    }
    p->info.steps = (uint32_t)d->n_steps;
    p->info.sets = (uint32_t)p->sets.size();
    p->info.narrow = narrow.top;
    p->info.instructions = (uint32_t)(p->code.size() / 2);
    p->info.taps = (uint32_t)d->n_taps;
    p->info.cells = (uint32_t)d->n_cells;
    while ((p->code.size() / 2) % CP_FETCH) emit(CP_NOP, 0, 0, 0, 0);
    return nullptr;
}

// ---- accumulate programs ("Accumulate programs" of bx_program.h): the constraint compiler's types, slot files and instructions, one
// list of vars, and term stores in place of mix steps ----
const char* compile_acc(const bx_acc_program_desc* d, bx_acc_program* p) {
    if (d->n_steps > BX_CONS_MAX_STEPS) return refuse("acc_program: %zu steps, more than BX_CONS_MAX_STEPS = %d", d->n_steps, BX_CONS_MAX_STEPS);
    if (d->n_taps > BX_CONS_MAX_TAPS) return refuse("acc_program: %zu taps, more than BX_CONS_MAX_TAPS = %d", d->n_taps, BX_CONS_MAX_TAPS);
    if (d->n_globals > BX_MAX_GLOBALS) return refuse("acc_program: n_globals %u is above BX_MAX_GLOBALS = %d", d->n_globals, BX_MAX_GLOBALS);
    if ((d->n_steps && !d->steps) || (d->n_taps && !d->taps)) return refuse("acc_program: null step or tap list");

    // ---- the tap list: ranges, and the kept columns in order of first appearance ----
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> kept_of;
    for (size_t t = 0; t < d->n_taps; ++t) {
        const bx_cons_tap& tp = d->taps[t];
        if (tp.group == 2) return refuse("acc_program: tap %zu: tap group 2 (accum): the program produces the accum group, it does not read it", t);
        if (tp.group > 2) return refuse("acc_program: tap %zu: tap group %u out of range (0 code, 1 data)", t, tp.group);
        if (tp.col > BX_CONS_MAX_COL) return refuse("acc_program: tap %zu: tap column %u out of range (at most %d)", t, tp.col, BX_CONS_MAX_COL);
        if (tp.back > BX_CONS_MAX_BACK) return refuse("acc_program: tap %zu: tap back %u out of range (at most %d)", t, tp.back, BX_CONS_MAX_BACK);
        const auto ins = kept_of.emplace(std::make_pair(tp.group, tp.col), (uint32_t)p->kept.size());
        if (ins.second) p->kept.push_back(bx_cons_tap{tp.group, tp.col, 0u});
        p->tap_kept.push_back(ins.first->second);
    }
    p->taps.assign(d->taps, d->taps + d->n_taps);

    // ---- pass 1: validation, types, sequences, last uses ----
    struct Var {
        bool ext = false;
        uint32_t slot = 0, last_use = 0;
    };
    std::vector<Var> fp;
    std::map<uint32_t, std::pair<size_t, bool>> seqs;  // sequence -> (the step that defines it, is it a sum)
    const auto use_fp = [&](size_t i, const char* what, uint32_t v) -> const char* {
        if (v >= fp.size()) return refuse("acc_program: step %zu: operand %s = %u refers to a later or missing fp var (%zu so far)", i, what, v, fp.size());
        fp[v].last_use = (uint32_t)i;
        return nullptr;
    };
    const auto define = [&](size_t i, uint32_t s, bool sum) -> const char* {
        if (s >= BX_ACC_MAX_SEQS) return refuse("acc_program: step %zu: sequence %u is not below BX_ACC_MAX_SEQS = %d", i, s, BX_ACC_MAX_SEQS);
        const auto ins = seqs.emplace(s, std::make_pair(i, sum));
        if (!ins.second) return refuse("acc_program: step %zu: sequence %u is defined a second time (first at step %zu)", i, s, ins.first->second.first);
        return nullptr;
    };
    static const char* const kForbidden[] = {"TRUE", "AND_EQZ", "AND_COND", "SET"};
    for (size_t i = 0; i < d->n_steps; ++i) {
        const bx_cons_step& s = d->steps[i];
        Var f;
        f.last_use = (uint32_t)i;
        switch (s.op) {
        case BX_CONS_CONST:
            if (s.a >= P) return refuse("acc_program: step %zu: constant %u is not below P", i, s.a);
            break;
        case BX_CONS_CONST_EXT:
            if (s.a >= P || s.b >= P || s.c >= P || s.d >= P)
                return refuse("acc_program: step %zu: ext constant (%u, %u, %u, %u) has a component not below P", i, s.a, s.b, s.c, s.d);
            f.ext = true;
            break;
        case BX_CONS_GET:
            if (s.a >= d->n_taps) return refuse("acc_program: step %zu: tap index %u out of range (%zu taps)", i, s.a, d->n_taps);
            break;
        case BX_CONS_GET_GLOBAL:
            if (s.a > 1) return refuse("acc_program: step %zu: GET_GLOBAL table %u out of range (0 globals, 1 mix)", i, s.a);
            if (s.a == 0 && s.b >= d->n_globals) return refuse("acc_program: step %zu: global index %u out of range (%u globals)", i, s.b, d->n_globals);
            if (s.a == 1 && s.b >= 4) return refuse("acc_program: step %zu: mix component %u out of range (an ext element has 4)", i, s.b);
            break;
        case BX_CONS_ADD:
        case BX_CONS_SUB:
        case BX_CONS_MUL:
            if (const char* m = use_fp(i, "a", s.a)) return m;
            if (const char* m = use_fp(i, "b", s.b)) return m;
            f.ext = fp[s.a].ext || fp[s.b].ext;
            break;
        case BX_CONS_SUM:
            if (const char* m = define(i, s.a, true)) return m;
            if (const char* m = use_fp(i, "m", s.b)) return m;
            if (const char* m = use_fp(i, "d", s.c)) return m;
            if (fp[s.b].ext) return refuse("acc_program: step %zu: SUM's m = %u is ext-typed; a multiplicity must be a base value", i, s.b);
            continue;  // appends nothing
        case BX_CONS_PROD:
            if (const char* m = define(i, s.a, false)) return m;
            if (const char* m = use_fp(i, "a", s.b)) return m;
            continue;
        default:
            if (s.op >= BX_CONS_TRUE && s.op <= BX_CONS_SET)
                return refuse("acc_program: step %zu: %s does not belong in an accumulate program (CONST, CONST_EXT, GET, GET_GLOBAL, ADD, SUB, MUL, SUM, PROD)", i,
                              kForbidden[s.op - BX_CONS_TRUE]);
            return refuse("acc_program: step %zu: unknown op %u", i, s.op);
        }
        fp.push_back(f);
    }
    if (seqs.empty()) return refuse("acc_program: the program defines no sequence (S = 0)");
    uint32_t expect = 0, sums = 0;
    bool prod_seen = false;
    for (const auto& kv : seqs) {  // in sequence order
        if (kv.first != expect) return refuse("acc_program: sequence %u is not defined: the sequences must be exactly 0 .. S-1 (sequence %u is defined)", expect, kv.first);
        ++expect;
        if (kv.second.second) {
            if (prod_seen)
                return refuse("acc_program: step %zu: SUM sequence %u is numbered above a PROD sequence: all sums come first, then all products", kv.second.first, kv.first);
            ++sums;
        } else {
            prod_seen = true;
        }
    }

    // ---- pass 2: slots by last use, and the stream ----
    SlotFile narrow, wide;
    const uint32_t scal_consts = d->n_globals + 4;  // where the constants start in `scal`
    const auto emit = [&](uint32_t op, uint32_t dst, uint32_t a, uint32_t b, uint32_t imm) {
        p->code.push_back(cp_w0(op, dst, a, b));
        p->code.push_back(cp_w1(0, imm));
    };
    uint32_t fi = 0;
    for (size_t i = 0; i < d->n_steps; ++i) {
        const bx_cons_step& s = d->steps[i];
        const uint32_t step = (uint32_t)i;
        // operands that die here give their slots back BEFORE the result takes one (dst may alias a source: executors read first)
        const auto drop = [&](uint32_t v) {
            if (fp[v].last_use == step) {
                (fp[v].ext ? wide : narrow).give(fp[v].slot);
                fp[v].last_use = NEVER - 1;  // an operand named twice is dropped once
            }
        };
        if (s.op == BX_CONS_SUM) {
            emit(fp[s.c].ext ? CP_TSUM_E : CP_TSUM_B, 0, fp[s.b].slot, fp[s.c].slot, s.a);
            drop(s.b);
            drop(s.c);
            continue;
        }
        if (s.op == BX_CONS_PROD) {
            emit(fp[s.b].ext ? CP_TPROD_E : CP_TPROD_B, 0, fp[s.b].slot, 0, s.a);
            drop(s.b);
            continue;
        }
        Var& f = fp[fi];
        const bool unused = f.last_use == step;
        uint32_t sa = 0, sb = 0;
        bool ea = false, eb = false;
        if (s.op >= BX_CONS_ADD) {
            sa = fp[s.a].slot, sb = fp[s.b].slot, ea = fp[s.a].ext, eb = fp[s.b].ext;
            drop(s.a);
            drop(s.b);
        }
        const uint32_t dst = f.slot = (f.ext ? wide : narrow).take();
        switch (s.op) {
        case BX_CONS_CONST:
            emit(CP_LD_B, dst, 0, 0, scal_consts + (uint32_t)p->consts.size());
            p->consts.push_back(fp_encode(s.a));
            break;
        case BX_CONS_CONST_EXT:
            emit(CP_LD_E, dst, 0, 0, scal_consts + (uint32_t)p->consts.size());
            for (uint32_t v : {s.a, s.b, s.c, s.d}) p->consts.push_back(fp_encode(v));
            break;
        case BX_CONS_GET: emit(CP_TAP, dst, 0, 0, s.a); break;
        case BX_CONS_GET_GLOBAL: emit(CP_LD_B, dst, 0, 0, s.a == 0 ? s.b : d->n_globals + s.b); break;
        case BX_CONS_ADD:
        case BX_CONS_MUL:
            if (!ea && !eb) emit(s.op == BX_CONS_ADD ? CP_ADD_BB : CP_MUL_BB, dst, sa, sb, 0);
            else if (ea && eb) emit(s.op == BX_CONS_ADD ? CP_ADD_EE : CP_MUL_EE, dst, sa, sb, 0);
            else emit(s.op == BX_CONS_ADD ? CP_ADD_EB : CP_MUL_EB, dst, ea ? sa : sb, ea ? sb : sa, 0);  // commutative: ext first
            break;
        default:  // BX_CONS_SUB
            emit(!ea && !eb ? CP_SUB_BB : (ea && eb ? CP_SUB_EE : (ea ? CP_SUB_EB : CP_SUB_BE)), dst, sa, sb, 0);
            break;
        }
        if (unused) (f.ext ? wide : narrow).give(dst);
        ++fi;
        if (narrow.peak > BX_CONS_MAX_NARROW || wide.peak > BX_CONS_MAX_WIDE) {
            const bool nw = narrow.peak > BX_CONS_MAX_NARROW;
            return refuse("acc_program: step %zu: the program needs %u live %s values, the limit is %d (BX_CONS_MAX_%s)", i, nw ? narrow.peak : wide.peak,
                          nw ? "narrow (base)" : "wide (ext)", nw ? BX_CONS_MAX_NARROW : BX_CONS_MAX_WIDE, nw ? "NARROW" : "WIDE");
        }
    }
    p->info.steps = (uint32_t)d->n_steps;
    p->info.sequences = (uint32_t)seqs.size();
    p->info.sums = sums;
    p->info.instructions = (uint32_t)(p->code.size() / 2);
    p->info.narrow = narrow.top;
    p->info.wide = wide.top;
    p->info.taps = (uint32_t)d->n_taps;
    p->info.kept = (uint32_t)p->kept.size();
    p->info.n_globals = d->n_globals;
    while ((p->code.size() / 2) % CP_FETCH) emit(CP_NOP, 0, 0, 0, 0);
    return nullptr;
}

}  // namespace

const char* acc_program_check_widths(const bx_acc_program* prog, const char* who, uint32_t w_code, uint32_t w_data) {
    for (size_t k = 0; k < prog->kept.size(); ++k) {
        const bx_cons_tap& t = prog->kept[k];
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
}  // namespace bx

extern "C" const char* bx_cons_program_create(const bx_cons_program_desc* desc, bx_cons_program** out) try {
    if (!desc || !out) return "bx_cons_program_create: null argument";
    *out = nullptr;
    bx_cons_program* p = new bx_cons_program();
    if (const char* e = bx::compile(desc, p)) {
        delete p;
        return e;
    }
    *out = p;
    return nullptr;
} catch (...) {
    return "bx_cons_program_create: out of host memory";
}

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

extern "C" const char* bx_cons_program_constraints_at(const bx_cons_program* prog, const bx_tap_reader* taps, const uint32_t poly_mix[4], const uint32_t mix[4],
                                                      const uint32_t* globals, uint32_t out[4]) try {
    using namespace bx;
    if (!prog || !taps || !taps->at || !poly_mix || !mix || !out) return "bx_cons_program_constraints_at: null argument";
    if (prog->info.n_globals && !globals) return "bx_cons_program_constraints_at: the program names globals and none were given";
    const uint32_t ng = prog->info.n_globals;
    std::vector<uint32_t> scal(ng + 4 + prog->consts.size());
    for (uint32_t i = 0; i < ng; ++i) scal[i] = globals[i];
    for (uint32_t i = 0; i < 4; ++i) scal[ng + i] = mix[i];
    std::copy(prog->consts.begin(), prog->consts.end(), scal.begin() + ng + 4);
    std::vector<Fp4> pows(prog->n_pows);
    const Fp4 pm{{poly_mix[0], poly_mix[1], poly_mix[2], poly_mix[3]}};
    pows[0] = f4_one();
    for (uint32_t e = 1; e < prog->n_pows; ++e) pows[e] = f4_mul(pows[e - 1], pm);
    // on the verifier every value is ext: the narrow file holds Fp4 too
    Fp4 nar[BX_CONS_MAX_NARROW], wid[BX_CONS_MAX_WIDE];
    for (Fp4& v : nar) v = f4_zero();
    for (Fp4& v : wid) v = f4_zero();
    const char* err = nullptr;
    const auto base = [](uint32_t w) { return Fp4{{w, 0u, 0u, 0u}}; };
    for (size_t pc = 0; pc < prog->code.size(); pc += 2) {
        const uint32_t w0 = prog->code[pc], w1 = prog->code[pc + 1];
        const uint32_t op = w0 & 0xFFu, dst = (w0 >> 8) & 0xFFu, a = (w0 >> 16) & 0xFFu, b = w0 >> 24, c = w1 & 0xFFu, imm = w1 >> 8;
        switch (op) {
        case CP_NOP: break;
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
        default: return "bx_cons_program_constraints_at: corrupt instruction stream";
        }
    }
    memcpy(out, wid[prog->ret_slot].c, 16);
    return err;
} catch (...) {
    return "bx_cons_program_constraints_at: out of host memory";
}

// ---- witness programs ----
extern "C" const char* bx_wit_program_create_counted(const bx_wit_program_desc* desc, const bx_wit_count* counts, size_t n_counts, bx_wit_program** out) try {
    if (!desc || !out) return "bx_wit_program_create: null argument";
    *out = nullptr;
    bx_wit_program* p = new bx_wit_program();
    if (const char* e = bx::compile_wit(desc, counts, n_counts, p)) {
        delete p;
        return e;
    }
    *out = p;
    return nullptr;
} catch (...) {
    return "bx_wit_program_create: out of host memory";
}

extern "C" const char* bx_wit_program_create(const bx_wit_program_desc* desc, bx_wit_program** out) { return bx_wit_program_create_counted(desc, nullptr, 0, out); }

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

extern "C" void bx_wit_program_destroy(bx_wit_program* prog) { delete prog; }

extern "C" const char* bx_wit_program_info_get(const bx_wit_program* prog, bx_wit_program_info* out) {
    if (!prog || !out) return "bx_wit_program_info_get: null argument";
    *out = prog->info;
    return nullptr;
}

extern "C" int bx_wit_program_derives(const bx_wit_program* prog, uint32_t col) {
    if (!prog) return 0;
    if (std::find(prog->sets.begin(), prog->sets.end(), col) != prog->sets.end()) return 1;
    for (const bx::WitCount& ct : prog->counts)
        if (ct.col == col) return 1;
    return 0;
}

extern "C" const char* bx_wit_program_run_host(const bx_wit_program* prog, uint32_t po2, const uint32_t* code, uint32_t w_code, uint32_t* data, uint32_t w_data) try {
    using namespace bx;
    if (!prog || (w_code && !code) || (w_data && !data)) return "bx_wit_program_run_host: null argument";
    if (po2 < 1 || po2 > 24) return "bx_wit_program_run_host: po2 must be in [1, 24]";
    if (const char* e = wit_program_check_widths(prog->max_col, prog->max_set, "bx_wit_program_run_host", w_code, w_data)) return e;
    if (const char* e = wit_program_check_counts(prog->counts, "bx_wit_program_run_host", po2, w_data)) return e;
    const size_t n = (size_t)1 << po2;
    // rows in any order: no row reads a word this run writes (derived cells are forwarded, never loaded)
    for (size_t r = 0; r < n; ++r) {
        uint32_t nar[BX_CONS_MAX_NARROW] = {};
        for (size_t pc = 0; pc < prog->code.size(); pc += 2) {
            const uint32_t w0 = prog->code[pc], w1 = prog->code[pc + 1];
            const uint32_t op = w0 & 0xFFu, dst = (w0 >> 8) & 0xFFu, a = (w0 >> 16) & 0xFFu, b = w0 >> 24, imm = w1 >> 8;
            if (dst >= BX_CONS_MAX_NARROW || a >= BX_CONS_MAX_NARROW || b >= BX_CONS_MAX_NARROW) return "bx_wit_program_run_host: corrupt instruction stream";
            switch (op) {
            case CP_NOP: break;
            case CP_LD_B: nar[dst] = prog->consts[imm]; break;
            case CP_TAP: {
                const bx_cons_tap& t = prog->taps[imm];
                const uint32_t* col = (t.group == 0 ? code : data) + (size_t)t.col * n;
                nar[dst] = col[((uint32_t)r - t.back) & (uint32_t)(n - 1)];  // N divides 2^32: the wrapped difference reduces properly
                break;
            }
            case CP_ADD_BB: nar[dst] = fp_add(nar[a], nar[b]); break;
            case CP_SUB_BB: nar[dst] = fp_sub(nar[a], nar[b]); break;
            case CP_MUL_BB: nar[dst] = fp_mul(nar[a], nar[b]); break;
            case CP_ST: data[(size_t)imm * n + r] = nar[a]; break;
            default: return "bx_wit_program_run_host: corrupt instruction stream";
            }
        }
    }
    // the counts, in list order, after every row: the device path's twin (clear, histogram over rows [0, rows), store)
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
extern "C" const char* bx_acc_program_create(const bx_acc_program_desc* desc, bx_acc_program** out) try {
    if (!desc || !out) return "bx_acc_program_create: null argument";
    *out = nullptr;
    bx_acc_program* p = new bx_acc_program();
    if (const char* e = bx::compile_acc(desc, p)) {
        delete p;
        return e;
    }
    *out = p;
    return nullptr;
} catch (...) {
    return "bx_acc_program_create: out of host memory";
}

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

extern "C" const char* bx_acc_program_run_host(const bx_acc_program* prog, uint32_t po2, const uint32_t* code, uint32_t w_code, const uint32_t* data,
                                               uint32_t w_data, const uint32_t* globals, const uint32_t mix[4], uint32_t* accum, uint32_t w_accum) try {
    using namespace bx;
    if (!prog || !mix || !accum || (w_code && !code) || (w_data && !data)) return "bx_acc_program_run_host: null argument";
    if (prog->info.n_globals && !globals) return "bx_acc_program_run_host: the program names globals and none were given";
    if (po2 < 1 || po2 > 24) return "bx_acc_program_run_host: po2 must be in [1, 24]";
    if (const char* e = acc_program_check_widths(prog, "bx_acc_program_run_host", w_code, w_data)) return e;
    const uint32_t S = prog->info.sequences, sums = prog->info.sums, ng = prog->info.n_globals;
    if (w_accum < 4 * S) return refuse("bx_acc_program_run_host: the program writes %u accum columns, the accum group has %u", 4 * S, w_accum);
    const size_t n = (size_t)1 << po2;
    std::vector<uint32_t> scal(ng + 4 + prog->consts.size());
    for (uint32_t i = 0; i < ng; ++i) scal[i] = globals[i];
    for (uint32_t i = 0; i < 4; ++i) scal[ng + i] = mix[i];
    std::copy(prog->consts.begin(), prog->consts.end(), scal.begin() + ng + 4);
    std::vector<Fp4> run((size_t)S * n, f4_zero());  // the device's run_ext: sequence-major AoS
    std::vector<uint32_t> mults((size_t)sums * n, 0u);
    // (1) the terms of every row
    for (size_t r = 0; r < n; ++r) {
        // a slot number is eight bits: files of 256 cannot be indexed out of bounds by any stream
        uint32_t nar[256] = {};
        Fp4 wid[256];
        for (Fp4& v : wid) v = f4_zero();
        for (size_t pc = 0; pc < prog->code.size(); pc += 2) {
            const uint32_t w0 = prog->code[pc], w1 = prog->code[pc + 1];
            const uint32_t op = w0 & 0xFFu, dst = (w0 >> 8) & 0xFFu, a = (w0 >> 16) & 0xFFu, b = w0 >> 24, imm = w1 >> 8;
            switch (op) {
            case CP_NOP: break;
            case CP_LD_B: nar[dst] = scal.at(imm); break;
            case CP_LD_E: wid[dst] = Fp4{{scal.at(imm), scal.at(imm + 1), scal.at(imm + 2), scal.at(imm + 3)}}; break;
            case CP_TAP: {
                const bx_cons_tap& t = prog->taps.at(imm);
                const uint32_t* col = (t.group == 0 ? code : data) + (size_t)t.col * n;
                nar[dst] = col[((uint32_t)r - t.back) & (uint32_t)(n - 1)];  // N divides 2^32: the wrapped difference reduces properly
                break;
            }
            case CP_ADD_BB: nar[dst] = fp_add(nar[a], nar[b]); break;
            case CP_SUB_BB: nar[dst] = fp_sub(nar[a], nar[b]); break;
            case CP_MUL_BB: nar[dst] = fp_mul(nar[a], nar[b]); break;
            case CP_ADD_EB: {
                Fp4 x = wid[a];
                x.c[0] = fp_add(x.c[0], nar[b]);
                wid[dst] = x;
                break;
            }
            case CP_SUB_EB: {
                Fp4 x = wid[a];
                x.c[0] = fp_sub(x.c[0], nar[b]);
                wid[dst] = x;
                break;
            }
            case CP_SUB_BE: wid[dst] = Fp4{{fp_sub(nar[a], wid[b].c[0]), fp_neg(wid[b].c[1]), fp_neg(wid[b].c[2]), fp_neg(wid[b].c[3])}}; break;
            case CP_MUL_EB: wid[dst] = f4_scale(wid[a], nar[b]); break;
            case CP_ADD_EE: wid[dst] = f4_add(wid[a], wid[b]); break;
            case CP_SUB_EE: wid[dst] = f4_sub(wid[a], wid[b]); break;
            case CP_MUL_EE: wid[dst] = f4_mul(wid[a], wid[b]); break;
            case CP_TSUM_B:
            case CP_TSUM_E:
                if (imm >= sums) return "bx_acc_program_run_host: corrupt instruction stream";
                run[(size_t)imm * n + r] = op == CP_TSUM_B ? Fp4{{nar[b], 0u, 0u, 0u}} : wid[b];
                mults[(size_t)imm * n + r] = nar[a];
                break;
            case CP_TPROD_B:
            case CP_TPROD_E:
                if (imm < sums || imm >= S) return "bx_acc_program_run_host: corrupt instruction stream";
                run[(size_t)imm * n + r] = op == CP_TPROD_B ? Fp4{{nar[a], 0u, 0u, 0u}} : wid[a];
                break;
            default: return "bx_acc_program_run_host: corrupt instruction stream";
            }
        }
    }
    // (2) m / d with 0 -> 0 and the running sums; (3) the running products; (4) sequence s, component k -> column 4 s + k
    for (uint32_t s = 0; s < S; ++s) {
        Fp4 acc = s < sums ? f4_zero() : f4_one();
        for (size_t r = 0; r < n; ++r) {
            const Fp4& v = run[(size_t)s * n + r];
            if (s < sums) acc = f4_add(acc, f4_is_zero(v) ? f4_zero() : f4_scale(f4_inv(v), mults[(size_t)s * n + r]));
            else acc = f4_mul(acc, v);
            for (uint32_t k = 0; k < 4; ++k) accum[(size_t)(4 * s + k) * n + r] = acc.c[k];
        }
    }
    return nullptr;
} catch (...) {
    return "bx_acc_program_run_host: out of host memory or a corrupt instruction stream";
}
