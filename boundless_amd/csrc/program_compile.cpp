// program_compile.cpp — the compiler of the three program kinds (include/bx_program.h is the normative text): from a step list to the
// instruction stream of cons_program.hpp.  ONE core (Core, below) owns what the kinds share: the limit and tap checks, the var table,
// the value steps CONST .. MUL with their base / ext opcodes, the slot allocation by last use, the peak check and the padding.  A kind
// is a description (Kind) plus the code for its own steps:
//   constraint programs   the mix vars (TRUE, AND_EQZ, AND_COND), the degrees and `ret`
//   witness programs      SET, forwarding of GETs, the global cells, the count list and the sort list
//   accumulate programs   SUM / PROD, the sequence rules and the kept list
// The ORDER in which a bad description is refused is part of the behaviour (tests/golden/progstream pins it): each kind's function
// below reads top to bottom in that order.
// No HIP: this translation unit compiles with plain g++ (the stand-alone checkers under tests/ run it under sanitizers).
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <memory>
#include <new>
#include <set>
#include <utility>

#include "fp.hpp"
#include "program_internal.hpp"

namespace bx {

const char* refuse(const char* fmt, ...) {
    thread_local char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    return msg;
}

namespace {

#define CP_TRY(expr)             \
    do {                         \
        const char* _m = (expr); \
        if (_m) return _m;       \
    } while (0)

constexpr uint32_t NEVER = 0xFFFFFFFFu;

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

// what tells the kinds apart where the core speaks or decides
struct Kind {
    const char* who;         // leads every refusal
    const char* lists;       // the lists a description may not leave NULL, as the refusal names them
    const char* no_accum;    // what is said of tap group 2 where it is not legal (NULL: it is)
    bool ext;                // ext values exist: CONST_EXT and GET_GLOBAL are value steps, a var has a type and there is a wide file
    bool degrees;            // a value's degree is bounded by BX_CONS_MAX_DEGREE
    uint32_t foreign;        // bit op: an op of another kind, refused as "does not belong" (every other op the kind lacks is unknown)
    const char* belongs;     // ... in what, and what does
    const char* wide_names;  // the wide file in the peak refusal
};
constexpr uint32_t bit(uint32_t op) { return 1u << op; }

// functions, not objects: the library's build compiles this file as HIP, where a namespace-scope constant would be emitted for the
// device too
const Kind& cons_kind() {
    static const Kind k{"cons_program", "step or tap", nullptr, true, true, 0, nullptr, "wide (ext and mix)"};
    return k;
}
const Kind& wit_kind() {
    static const Kind k{"wit_program", "step, tap or cell", " does not exist when the witness is generated", false, false,
                        bit(BX_CONS_CONST_EXT) | bit(BX_CONS_GET_GLOBAL) | bit(BX_CONS_TRUE) | bit(BX_CONS_AND_EQZ) | bit(BX_CONS_AND_COND),
                        "a witness program (CONST, GET, ADD, SUB, MUL, SET)", ""};
    return k;
}
const Kind& acc_kind() {
    static const Kind k{"acc_program", "step or tap", ": the program produces the accum group, it does not read it", true, false,
                        bit(BX_CONS_TRUE) | bit(BX_CONS_AND_EQZ) | bit(BX_CONS_AND_COND) | bit(BX_CONS_SET),
                        "an accumulate program (CONST, CONST_EXT, GET, GET_GLOBAL, ADD, SUB, MUL, SUM, PROD)", "wide (ext)"};
    return k;
}

// an fp var: a value in a slot of its type's file, or — a witness program's GET of a derived column after its SET — another name of
// the var that was stored
struct Var {
    bool ext = false;
    uint32_t degree = 0;
    uint32_t root = 0;  // the var that holds the value (itself unless forwarded)
    uint32_t slot = 0, last_use = 0;  // of a root.  last_use: the step that reads it last (its own step if none does)
};

struct Core {
    const Kind& k;
    const bx_cons_step* steps;
    size_t n_steps;
    const bx_cons_tap* taps;
    size_t n_taps;
    uint32_t n_globals;    // 0 for a kind without globals
    uint32_t scal_consts;  // where the constants start in `scal`
    std::vector<uint32_t>& code;
    std::vector<uint32_t>& consts;
    std::vector<Var> fp;
    SlotFile narrow, wide;

    template <class Desc, class Prog>
    Core(const Kind& kind, const Desc* d, uint32_t globals, uint32_t consts_at, Prog* p)
        : k(kind), steps(d->steps), n_steps(d->n_steps), taps(d->taps), n_taps(d->n_taps), n_globals(globals), scal_consts(consts_at), code(p->code), consts(p->consts) {}

    // ---- the limits, in the order they are judged; a witness program's public words are its cells ----
    const char* limits(const void* cells = nullptr, size_t n_cells = 0) const {
        if (n_steps > BX_CONS_MAX_STEPS) return refuse("%s: %zu steps, more than BX_CONS_MAX_STEPS = %d", k.who, n_steps, BX_CONS_MAX_STEPS);
        if (n_taps > BX_CONS_MAX_TAPS) return refuse("%s: %zu taps, more than BX_CONS_MAX_TAPS = %d", k.who, n_taps, BX_CONS_MAX_TAPS);
        if (n_globals > BX_MAX_GLOBALS) return refuse("%s: n_globals %u is above BX_MAX_GLOBALS = %d", k.who, n_globals, BX_MAX_GLOBALS);
        if (n_cells > BX_MAX_GLOBALS) return refuse("%s: %zu global cells, more than BX_MAX_GLOBALS = %d", k.who, n_cells, BX_MAX_GLOBALS);
        if ((n_steps && !steps) || (n_taps && !taps) || (n_cells && !cells)) return refuse("%s: null %s list", k.who, k.lists);
        return nullptr;
    }

    // ---- the tap list: ranges; `each(t, tap)` is the kind's own look at a tap that passed them ----
    template <class Each>
    const char* check_taps(Each each) const {
        for (size_t t = 0; t < n_taps; ++t) {
            const bx_cons_tap& tp = taps[t];
            if (tp.group == 2 && k.no_accum) return refuse("%s: tap %zu: tap group 2 (accum)%s", k.who, t, k.no_accum);
            if (tp.group > 2) return refuse("%s: tap %zu: tap group %u out of range (0 code, 1 data%s)", k.who, t, tp.group, k.no_accum ? "" : ", 2 accum");
            if (tp.col > BX_CONS_MAX_COL) return refuse("%s: tap %zu: tap column %u out of range (at most %d)", k.who, t, tp.col, BX_CONS_MAX_COL);
            if (tp.back > BX_CONS_MAX_BACK) return refuse("%s: tap %zu: tap back %u out of range (at most %d)", k.who, t, tp.back, BX_CONS_MAX_BACK);
            CP_TRY(each(t, tp));
        }
        return nullptr;
    }

    // ---- pass 1: validation, types, degrees, last uses ----
    Var& at(uint32_t v) { return fp[fp[v].root]; }  // the var that holds v's value
    bool is_value(uint32_t op) const { return op <= BX_CONS_MUL && (k.ext || (op != BX_CONS_CONST_EXT && op != BX_CONS_GET_GLOBAL)); }
    const char* use(size_t i, const char* what, uint32_t v) {
        if (v >= fp.size()) return refuse("%s: step %zu: operand %s = %u refers to a later or missing fp var (%zu so far)", k.who, i, what, v, fp.size());
        at(v).last_use = (uint32_t)i;
        return nullptr;
    }
    // an op that is neither a value step nor one of the kind's own
    const char* no_such_op(size_t i, uint32_t op) const {
        static const char* const kOpNames[] = {"CONST", "CONST_EXT", "GET", "GET_GLOBAL", "ADD", "SUB", "MUL", "TRUE", "AND_EQZ", "AND_COND", "SET", "SUM", "PROD"};
        if (op < sizeof kOpNames / sizeof kOpNames[0] && (k.foreign & bit(op))) return refuse("%s: step %zu: %s does not belong in %s", k.who, i, kOpNames[op], k.belongs);
        return refuse("%s: step %zu: unknown op %u", k.who, i, op);
    }
    const char* degree_ok(size_t i, uint32_t degree) const {
        if (k.degrees && degree > BX_CONS_MAX_DEGREE)
            return refuse("%s: step %zu: degree %u is above BX_CONS_MAX_DEGREE = %d (the quotient would not fit the 4N check evaluations)", k.who, i, degree,
                          BX_CONS_MAX_DEGREE);
        return nullptr;
    }
    // `get(i, var)`: the kind's own look at a GET whose tap index is in range (forwarding); `own(i, step)`: every step that is no
    // value step
    template <class Get, class Own>
    const char* validate(Get get, Own own) {
        for (size_t i = 0; i < n_steps; ++i) {
            const bx_cons_step& s = steps[i];
            if (!is_value(s.op)) {
                CP_TRY(own(i, s));
                continue;
            }
            Var f;
            f.root = (uint32_t)fp.size();
            f.last_use = (uint32_t)i;
            switch (s.op) {
            case BX_CONS_CONST:
                if (s.a >= P) return refuse("%s: step %zu: constant %u is not below P", k.who, i, s.a);
                break;
            case BX_CONS_CONST_EXT:
                if (s.a >= P || s.b >= P || s.c >= P || s.d >= P)
                    return refuse("%s: step %zu: ext constant (%u, %u, %u, %u) has a component not below P", k.who, i, s.a, s.b, s.c, s.d);
                f.ext = true;
                break;
            case BX_CONS_GET:
                if (s.a >= n_taps) return refuse("%s: step %zu: tap index %u out of range (%zu taps)", k.who, i, s.a, n_taps);
                f.degree = 1;
                CP_TRY(get(i, f));
                break;
            case BX_CONS_GET_GLOBAL:
                if (s.a > 1) return refuse("%s: step %zu: GET_GLOBAL table %u out of range (0 globals, 1 mix)", k.who, i, s.a);
                if (s.a == 0 && s.b >= n_globals) return refuse("%s: step %zu: global index %u out of range (%u globals)", k.who, i, s.b, n_globals);
                if (s.a == 1 && s.b >= 4) return refuse("%s: step %zu: mix component %u out of range (an ext element has 4)", k.who, i, s.b);
                break;
            default:  // BX_CONS_ADD, BX_CONS_SUB, BX_CONS_MUL
                CP_TRY(use(i, "a", s.a));
                CP_TRY(use(i, "b", s.b));
                f.ext = fp[s.a].ext || fp[s.b].ext;
                f.degree = s.op == BX_CONS_MUL ? fp[s.a].degree + fp[s.b].degree : std::max(fp[s.a].degree, fp[s.b].degree);
                break;
            }
            CP_TRY(degree_ok(i, f.degree));
            fp.push_back(f);
        }
        return nullptr;
    }
    template <class Own>
    const char* validate(Own own) {
        return validate([](size_t, Var&) -> const char* { return nullptr; }, own);
    }

    // ---- pass 2: slots by last use, and the stream ----
    void emit(uint32_t op, uint32_t dst, uint32_t a, uint32_t b, uint32_t c, uint32_t imm) {
        code.push_back(cp_w0(op, dst, a, b));
        code.push_back(cp_w1(c, imm));
    }
    SlotFile& file(const Var& v) { return v.ext ? wide : narrow; }
    // an operand that dies at `step` gives its slot back BEFORE the result takes one (dst may alias a source: executors read first)
    void drop(uint32_t v, uint32_t step) {
        Var& r = at(v);
        if (r.last_use == step) {
            file(r).give(r.slot);
            r.last_use = NEVER - 1;  // an operand named twice is dropped once
        }
    }
    void value(uint32_t step, const bx_cons_step& s, uint32_t fi) {
        Var& f = fp[fi];
        if (f.root != fi) return drop(fi, step);  // a forwarded GET compiles to nothing; one that nothing reads afterwards ends the stored value's life
        const bool unused = f.last_use == step;
        uint32_t sa = 0, sb = 0;
        bool ea = false, eb = false;
        if (s.op >= BX_CONS_ADD) {
            sa = at(s.a).slot, sb = at(s.b).slot, ea = at(s.a).ext, eb = at(s.b).ext;
            drop(s.a, step);
            drop(s.b, step);
        }
        const uint32_t dst = f.slot = file(f).take();
        switch (s.op) {
        case BX_CONS_CONST:
            emit(CP_LD_B, dst, 0, 0, 0, scal_consts + (uint32_t)consts.size());
            consts.push_back(fp_encode(s.a));
            break;
        case BX_CONS_CONST_EXT:
            emit(CP_LD_E, dst, 0, 0, 0, scal_consts + (uint32_t)consts.size());
            for (uint32_t v : {s.a, s.b, s.c, s.d}) consts.push_back(fp_encode(v));
            break;
        case BX_CONS_GET: emit(CP_TAP, dst, 0, 0, 0, s.a); break;
        case BX_CONS_GET_GLOBAL: emit(CP_LD_B, dst, 0, 0, 0, s.a == 0 ? s.b : n_globals + s.b); break;
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
        if (unused) file(f).give(dst);
    }
    // `own(step, s)` emits a step that is no value step
    template <class Own>
    const char* allocate(Own own) {
        uint32_t fi = 0;
        for (size_t i = 0; i < n_steps; ++i) {
            const bx_cons_step& s = steps[i];
            if (is_value(s.op)) value((uint32_t)i, s, fi++);
            else own((uint32_t)i, s);
            if (narrow.peak <= BX_CONS_MAX_NARROW && wide.peak <= BX_CONS_MAX_WIDE) continue;
            if (!k.ext) return refuse("%s: step %zu: the program needs %u live values, the limit is %d (BX_CONS_MAX_NARROW)", k.who, i, narrow.peak, BX_CONS_MAX_NARROW);
            const bool nw = narrow.peak > BX_CONS_MAX_NARROW;
            return refuse("%s: step %zu: the program needs %u live %s values, the limit is %d (BX_CONS_MAX_%s)", k.who, i, nw ? narrow.peak : wide.peak,
                          nw ? "narrow (base)" : k.wide_names, nw ? BX_CONS_MAX_NARROW : BX_CONS_MAX_WIDE, nw ? "NARROW" : "WIDE");
        }
        return nullptr;
    }
    // the stream's length before the padding, which fills it to whole fetches
    uint32_t pad() {
        const uint32_t instructions = (uint32_t)(code.size() / 2);
        while ((code.size() / 2) % CP_FETCH) emit(CP_NOP, 0, 0, 0, 0, 0);
        return instructions;
    }
};

// ---- constraint programs: a second list, of mix vars (tot in a wide slot, mul a statically known power of poly_mix) ----
struct MixVar {
    uint32_t exp = 0, degree = 0, slot = 0, last_use = 0;
};

const char* compile(const bx_cons_program_desc* d, bx_cons_program* p) {
    Core c(cons_kind(), d, d->n_globals, d->n_globals + 4, p);
    CP_TRY(c.limits());
    std::map<std::pair<uint32_t, uint32_t>, std::set<uint32_t>> backs;  // the tap set of every named column
    CP_TRY(c.check_taps([&](size_t t, const bx_cons_tap& tp) -> const char* {
        std::set<uint32_t>& s = backs[{tp.group, tp.col}];
        s.insert(0u);
        s.insert(tp.back);
        if (s.size() > BX_MAX_TAPS)
            return refuse("cons_program: tap %zu: more than BX_MAX_TAPS = %d distinct backs on column %u of group %u", t, BX_MAX_TAPS, tp.col, tp.group);
        p->max_col[tp.group] = std::max(p->max_col[tp.group], tp.col + 1);
        return nullptr;
    }));
    p->taps.assign(d->taps, d->taps + d->n_taps);

    std::vector<MixVar> mix;
    const auto use_mix = [&](size_t i, const char* what, uint32_t v) -> const char* {
        if (v >= mix.size()) return refuse("cons_program: step %zu: operand %s = %u refers to a later or missing mix var (%zu so far)", i, what, v, mix.size());
        mix[v].last_use = (uint32_t)i;
        return nullptr;
    };
    CP_TRY(c.validate([&](size_t i, const bx_cons_step& s) -> const char* {
        MixVar m;
        m.last_use = (uint32_t)i;
        switch (s.op) {
        case BX_CONS_TRUE: break;
        case BX_CONS_AND_EQZ:
            CP_TRY(use_mix(i, "a", s.a));
            CP_TRY(c.use(i, "b", s.b));
            m.exp = mix[s.a].exp + 1;
            m.degree = std::max(mix[s.a].degree, c.fp[s.b].degree);
            break;
        case BX_CONS_AND_COND:
            CP_TRY(use_mix(i, "a", s.a));
            CP_TRY(c.use(i, "b", s.b));
            CP_TRY(use_mix(i, "c", s.c));
            m.exp = mix[s.a].exp + mix[s.c].exp;
            m.degree = std::max(mix[s.a].degree, c.fp[s.b].degree + mix[s.c].degree);
            break;
        default: return c.no_such_op(i, s.op);
        }
        CP_TRY(c.degree_ok(i, m.degree));
        if (m.exp > BX_CONS_MAX_STEPS) return refuse("cons_program: step %zu: %u constraints, more than BX_CONS_MAX_STEPS = %d", i, m.exp, BX_CONS_MAX_STEPS);
        mix.push_back(m);
        return nullptr;
    }));
    if (d->ret >= mix.size()) return refuse("cons_program: ret = %u is not a mix var (%zu mix vars)", d->ret, mix.size());
    mix[d->ret].last_use = NEVER;

    uint32_t n_pows = 1, mi = 0;
    CP_TRY(c.allocate([&](uint32_t step, const bx_cons_step& s) {
        const auto drop_mix = [&](uint32_t v) {
            if (mix[v].last_use == step) {
                c.wide.give(mix[v].slot);
                mix[v].last_use = NEVER - 1;
            }
        };
        MixVar& m = mix[mi++];
        const bool unused = m.last_use == step;
        if (s.op == BX_CONS_TRUE) {
            m.slot = c.wide.take();
            c.emit(CP_ZERO, m.slot, 0, 0, 0, 0);
        } else {
            const uint32_t sx = mix[s.a].slot, sy = c.fp[s.b].slot, e = mix[s.a].exp;
            const bool ey = c.fp[s.b].ext;
            const uint32_t sc = s.op == BX_CONS_AND_COND ? mix[s.c].slot : 0u;
            drop_mix(s.a);
            c.drop(s.b, step);
            if (s.op == BX_CONS_AND_COND) drop_mix(s.c);
            m.slot = c.wide.take();
            if (s.op == BX_CONS_AND_EQZ) c.emit(ey ? CP_EQZ_E : CP_EQZ_B, m.slot, sx, sy, 0, e);
            else c.emit(ey ? CP_COND_E : CP_COND_B, m.slot, sx, sy, sc, e);
            n_pows = std::max(n_pows, e + 1);
        }
        if (unused) c.wide.give(m.slot);
    }));
    p->info.steps = (uint32_t)d->n_steps;
    p->info.constraints = mix[d->ret].exp;
    p->info.degree = mix[d->ret].degree;
    p->info.narrow = c.narrow.top;
    p->info.wide = c.wide.top;
    p->info.instructions = c.pad();
    p->info.taps = (uint32_t)d->n_taps;
    p->info.n_globals = d->n_globals;
    p->n_pows = n_pows;
    p->ret_slot = mix[d->ret].slot;
    return nullptr;
}

// ---- witness programs ("Witness programs" of bx_program.h): narrow values only, SET, forwarding, cells and counts ----
// the count list ("multiplicity columns"): every rule but the shape-dependent ones (wit_program_check_counts)
const char* check_counts(const bx_wit_program_desc* d, const bx_wit_count* counts, size_t n_counts, const std::map<uint32_t, size_t>& set_at, bx_wit_program* p) {
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
    return nullptr;
}

// the sort list ("sorted columns"): every rule but the shape-dependent ones (wit_program_check_sorts).  After check_counts: p->counts
// is what a dest and a source are held against.
const char* check_sorts(const bx_wit_program_desc* d, const bx_wit_sort* sorts, size_t n_sorts, const std::map<uint32_t, size_t>& set_at, bx_wit_program* p) {
    if (n_sorts > BX_WIT_MAX_SORTS) return refuse("wit_program: %zu sorts, more than BX_WIT_MAX_SORTS = %d", n_sorts, BX_WIT_MAX_SORTS);
    if (n_sorts && !sorts) return refuse("wit_program: null sort list");
    std::map<uint32_t, size_t> count_of, dest_of, source_of;  // data column -> the count that fills it / the first sort that writes it / reads it
    for (size_t k = 0; k < p->counts.size(); ++k) count_of.emplace(p->counts[k].col, k);
    for (size_t k = 0; k < n_sorts; ++k) {
        const bx_wit_sort& s = sorts[k];
        if (s.n_cols == 0) return refuse("wit_program: sort %zu: no sources", k);
        if (s.n_cols > BX_WIT_MAX_SORT_COLS) return refuse("wit_program: sort %zu: %u sources, more than BX_WIT_MAX_SORT_COLS = %d", k, s.n_cols, BX_WIT_MAX_SORT_COLS);
        if (s.n_keys == 0) return refuse("wit_program: sort %zu: n_keys is 0", k);
        if (s.n_keys > BX_WIT_MAX_SORT_KEYS) return refuse("wit_program: sort %zu: %u keys, more than BX_WIT_MAX_SORT_KEYS = %d", k, s.n_keys, BX_WIT_MAX_SORT_KEYS);
        if (s.n_keys > s.n_cols) return refuse("wit_program: sort %zu: %u keys, above its %u sources", k, s.n_keys, s.n_cols);
        if (!s.bits || !s.sources || !s.dests) return refuse("wit_program: sort %zu: null bits, source or dest list", k);
        if (s.rows > (1u << 24)) return refuse("wit_program: sort %zu: rows %u is above 2^24, the largest trace", k, s.rows);
        WitSort ws;
        ws.rows = s.rows;
        uint32_t total = 0;
        for (uint32_t q = 0; q < s.n_keys; ++q) {
            if (s.bits[q] == 0 || s.bits[q] > 31) return refuse("wit_program: sort %zu: key %u: bits %u is outside [1, 31]", k, q, s.bits[q]);
            total += s.bits[q];
            ws.bits.push_back(s.bits[q]);
        }
        if (total > BX_WIT_MAX_SORT_BITS) return refuse("wit_program: sort %zu: the keys have %u bits, more than BX_WIT_MAX_SORT_BITS = %d", k, total, BX_WIT_MAX_SORT_BITS);
        for (uint32_t q = 0; q < s.n_cols; ++q) {
            const uint32_t src = s.sources[q];
            if (src > BX_CONS_MAX_COL) return refuse("wit_program: sort %zu: source %u: data column %u out of range (at most %d)", k, q, src, BX_CONS_MAX_COL);
            if (std::find(ws.sources.begin(), ws.sources.end(), src) != ws.sources.end()) return refuse("wit_program: sort %zu: source column %u is named twice", k, src);
            const auto ct = count_of.find(src);
            if (ct != count_of.end())
                return refuse("wit_program: sort %zu: source column %u is the column of count %zu: the counts run after the sorts", k, src, ct->second);
            ws.sources.push_back(src);
            source_of.emplace(src, k);
        }
        for (uint32_t q = 0; q < s.n_cols; ++q) {
            const uint32_t dst = s.dests[q];
            if (dst > BX_CONS_MAX_COL) return refuse("wit_program: sort %zu: dest %u: data column %u out of range (at most %d)", k, q, dst, BX_CONS_MAX_COL);
            const auto ins = dest_of.emplace(dst, k);
            if (!ins.second) return refuse("wit_program: sort %zu: dest column %u is already a dest of sort %zu", k, dst, ins.first->second);
            const auto st = set_at.find(dst);
            if (st != set_at.end()) return refuse("wit_program: sort %zu: dest column %u is also SET (step %zu)", k, dst, st->second);
            const auto ct = count_of.find(dst);
            if (ct != count_of.end()) return refuse("wit_program: sort %zu: dest column %u is the column of count %zu", k, dst, ct->second);
            ws.dests.push_back(dst);
        }
        p->sorts.push_back(std::move(ws));
    }
    for (size_t k = 0; k < p->sorts.size(); ++k)  // in list order: the first sort with such a dest is the one named
        for (uint32_t dst : p->sorts[k].dests) {
            const auto src = source_of.find(dst);
            if (src != source_of.end()) return refuse("wit_program: sort %zu: dest column %u is a source of sort %zu", k, dst, src->second);
        }
    if (!dest_of.empty())
        for (size_t i = 0; i < d->n_steps; ++i) {
            const bx_cons_step& s = d->steps[i];
            if (s.op != BX_CONS_GET || s.a >= d->n_taps || d->taps[s.a].group != 1) continue;
            const auto it = dest_of.find(d->taps[s.a].col);
            if (it != dest_of.end())
                return refuse("wit_program: sort %zu: dest column %u is read by the GET of step %zu: a sorted column does not exist while the program runs", it->second,
                              it->first, i);
        }
    return nullptr;
}

const char* compile_wit(const bx_wit_program_desc* d, const bx_wit_count* counts, size_t n_counts, const bx_wit_sort* sorts, size_t n_sorts, bx_wit_program* p) {
    Core c(wit_kind(), d, 0, 0, p);  // `scal` is the constants alone
    CP_TRY(c.limits(d->cells, d->n_cells));
    CP_TRY(c.check_taps([&](size_t, const bx_cons_tap& tp) -> const char* {
        p->max_col[tp.group] = std::max(p->max_col[tp.group], tp.col + 1);
        return nullptr;
    }));
    p->taps.assign(d->taps, d->taps + d->n_taps);
    std::set<uint32_t> named;
    for (size_t k = 0; k < d->n_cells; ++k) {
        const bx_wit_global_cell& g = d->cells[k];
        if (g.global >= BX_MAX_GLOBALS) return refuse("wit_program: cell %zu: global index %u is not below BX_MAX_GLOBALS = %d", k, g.global, BX_MAX_GLOBALS);
        if (g.col > BX_CONS_MAX_COL) return refuse("wit_program: cell %zu: data column %u out of range (at most %d)", k, g.col, BX_CONS_MAX_COL);
        if (!named.insert(g.global).second) return refuse("wit_program: cell %zu: global index %u is named twice", k, g.global);
    }
    p->cells.assign(d->cells, d->cells + d->n_cells);

    // which data columns are derived, and where
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

    CP_TRY(c.validate(
        [&](size_t i, Var& f) -> const char* {
            const bx_cons_tap& tp = d->taps[d->steps[i].a];
            const auto it = tp.group == 1 ? set_at.find(tp.col) : set_at.end();
            if (it == set_at.end()) return nullptr;  // a free cell: a memory read
            if (tp.back > 0)
                return refuse("wit_program: step %zu: GET of derived data column %u with back %u: another row's value may not have been written yet", i, tp.col, tp.back);
            if (it->second > i) return refuse("wit_program: step %zu: GET of derived data column %u before its SET at step %zu", i, tp.col, it->second);
            f.root = c.fp[d->steps[it->second].b].root;  // forwarded: the var that was stored (its SET has been validated: it is earlier)
            c.fp[f.root].last_use = (uint32_t)i;
            return nullptr;
        },
        [&](size_t i, const bx_cons_step& s) -> const char* {
            if (s.op != BX_CONS_SET) return c.no_such_op(i, s.op);
            return c.use(i, "b", s.b);  // appends nothing
        }));
    // after the step list, so that a description with a bad step is refused for that step
    CP_TRY(check_counts(d, counts, n_counts, set_at, p));
    CP_TRY(check_sorts(d, sorts, n_sorts, set_at, p));

    CP_TRY(c.allocate([&](uint32_t step, const bx_cons_step& s) {
        c.emit(CP_ST, 0, c.at(s.b).slot, 0, 0, s.a);
        c.drop(s.b, step);
    }));
    p->info.steps = (uint32_t)d->n_steps;
    p->info.sets = (uint32_t)p->sets.size();
    p->info.narrow = c.narrow.top;
    p->info.instructions = c.pad();
    p->info.taps = (uint32_t)d->n_taps;
    p->info.cells = (uint32_t)d->n_cells;
    return nullptr;
}

// ---- accumulate programs ("Accumulate programs" of bx_program.h): the constraint compiler's types, term stores in place of mix steps ----
const char* compile_acc(const bx_acc_program_desc* d, bx_acc_program* p) {
    Core c(acc_kind(), d, d->n_globals, d->n_globals + 4, p);
    CP_TRY(c.limits());
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> kept_of;  // the kept columns, in order of first appearance
    CP_TRY(c.check_taps([&](size_t, const bx_cons_tap& tp) -> const char* {
        const auto ins = kept_of.emplace(std::make_pair(tp.group, tp.col), (uint32_t)p->kept.size());
        if (ins.second) p->kept.push_back(bx_cons_tap{tp.group, tp.col, 0u});
        p->tap_kept.push_back(ins.first->second);
        return nullptr;
    }));
    p->taps.assign(d->taps, d->taps + d->n_taps);

    enum : int { SEQ_SUM, SEQ_PROD, SEQ_RATIO };
    std::map<uint32_t, std::pair<size_t, int>> seqs;  // sequence -> (the step that defines it, its kind)
    const auto define = [&](size_t i, uint32_t s, int kind) -> const char* {
        if (s >= BX_ACC_MAX_SEQS) return refuse("acc_program: step %zu: sequence %u is not below BX_ACC_MAX_SEQS = %d", i, s, BX_ACC_MAX_SEQS);
        const auto ins = seqs.emplace(s, std::make_pair(i, kind));
        if (!ins.second) return refuse("acc_program: step %zu: sequence %u is defined a second time (first at step %zu)", i, s, ins.first->second.first);
        return nullptr;
    };
    CP_TRY(c.validate([&](size_t i, const bx_cons_step& s) -> const char* {  // both append nothing
        switch (s.op) {
        case BX_CONS_SUM:
            CP_TRY(define(i, s.a, SEQ_SUM));
            CP_TRY(c.use(i, "m", s.b));
            CP_TRY(c.use(i, "d", s.c));
            if (c.fp[s.b].ext) return refuse("acc_program: step %zu: SUM's m = %u is ext-typed; a multiplicity must be a base value", i, s.b);
            return nullptr;
        case BX_CONS_PROD:
            CP_TRY(define(i, s.a, SEQ_PROD));
            return c.use(i, "a", s.b);
        case BX_CONS_RATIO:
            CP_TRY(define(i, s.a, SEQ_RATIO));
            CP_TRY(c.use(i, "a", s.b));
            return c.use(i, "b", s.c);
        default: return c.no_such_op(i, s.op);
        }
    }));
    if (seqs.empty()) return refuse("acc_program: the program defines no sequence (S = 0)");
    uint32_t expect = 0, sums = 0, ratios = 0;
    bool prod_seen = false;
    const std::pair<const uint32_t, std::pair<size_t, int>>* ratio_seen = nullptr;  // the lowest-numbered RATIO
    for (const auto& kv : seqs) {  // in sequence order
        if (kv.first != expect) return refuse("acc_program: sequence %u is not defined: the sequences must be exactly 0 .. S-1 (sequence %u is defined)", expect, kv.first);
        ++expect;
        const int kind = kv.second.second;
        if (kind == SEQ_SUM && prod_seen)
            return refuse("acc_program: step %zu: SUM sequence %u is numbered above a PROD sequence: all sums come first, then all products", kv.second.first, kv.first);
        if (kind != SEQ_RATIO && ratio_seen)
            return refuse("acc_program: step %zu: %s sequence %u is numbered above a RATIO sequence (step %zu: RATIO sequence %u is numbered below a %s sequence): "
                          "all sums come first, then all products, then all ratios",
                          kv.second.first, kind == SEQ_SUM ? "SUM" : "PROD", kv.first, ratio_seen->second.first, ratio_seen->first, kind == SEQ_SUM ? "SUM" : "PROD");
        if (kind == SEQ_SUM) ++sums;
        else if (kind == SEQ_PROD) prod_seen = true;
        else {
            if (!ratio_seen) ratio_seen = &kv;
            ++ratios;
        }
    }

    CP_TRY(c.allocate([&](uint32_t step, const bx_cons_step& s) {
        if (s.op == BX_CONS_SUM) {
            c.emit(c.fp[s.c].ext ? CP_TSUM_E : CP_TSUM_B, 0, c.fp[s.b].slot, c.fp[s.c].slot, 0, s.a);
            c.drop(s.b, step);
            c.drop(s.c, step);
        } else if (s.op == BX_CONS_PROD) {
            c.emit(c.fp[s.b].ext ? CP_TPROD_E : CP_TPROD_B, 0, c.fp[s.b].slot, 0, 0, s.a);
            c.drop(s.b, step);
        } else {  // RATIO: the numerator where a product's factor goes, the denominator R sequences further on
            c.emit(c.fp[s.b].ext ? CP_TPROD_E : CP_TPROD_B, 0, c.fp[s.b].slot, 0, 0, s.a);
            c.emit(c.fp[s.c].ext ? CP_TDEN_E : CP_TDEN_B, 0, c.fp[s.c].slot, 0, 0, s.a + ratios);
            c.drop(s.b, step);
            c.drop(s.c, step);
        }
    }));
    p->info.steps = (uint32_t)d->n_steps;
    p->info.sequences = (uint32_t)seqs.size();
    p->info.sums = sums;
    p->ratios = ratios;
    p->info.instructions = c.pad();
    p->info.narrow = c.narrow.top;
    p->info.wide = c.wide.top;
    p->info.taps = (uint32_t)d->n_taps;
    p->info.kept = (uint32_t)p->kept.size();
    p->info.n_globals = d->n_globals;
    return nullptr;
}
// create: compile into a fresh program, which is the caller's only when nothing was refused.  What the compiler wrote must pass the
// check every consumer makes (program_fits): the two are written apart, so each holds the other to the operand table
template <class Prog, class Compile>
const char* create(const Kind& k, Prog** out, Compile compile_into) {
    *out = nullptr;
    std::unique_ptr<Prog> p(new Prog());
    CP_TRY(compile_into(p.get()));
    if (!program_fits(p.get())) return refuse("%s: internal error: the compiled stream does not pass program_fits", k.who);
    *out = p.release();
    return nullptr;
}
#undef CP_TRY

}  // namespace
}  // namespace bx

extern "C" const char* bx_cons_program_create(const bx_cons_program_desc* desc, bx_cons_program** out) try {
    if (!desc || !out) return "bx_cons_program_create: null argument";
    return bx::create(bx::cons_kind(), out, [&](bx_cons_program* p) { return bx::compile(desc, p); });
} catch (...) {
    return "bx_cons_program_create: out of host memory";
}

extern "C" const char* bx_wit_program_create_sorted(const bx_wit_program_desc* desc, const bx_wit_count* counts, size_t n_counts, const bx_wit_sort* sorts,
                                                    size_t n_sorts, bx_wit_program** out) try {
    if (!desc || !out) return "bx_wit_program_create: null argument";
    return bx::create(bx::wit_kind(), out, [&](bx_wit_program* p) { return bx::compile_wit(desc, counts, n_counts, sorts, n_sorts, p); });
} catch (...) {
    return "bx_wit_program_create: out of host memory";
}

extern "C" const char* bx_wit_program_create_counted(const bx_wit_program_desc* desc, const bx_wit_count* counts, size_t n_counts, bx_wit_program** out) {
    return bx_wit_program_create_sorted(desc, counts, n_counts, nullptr, 0, out);
}

extern "C" const char* bx_wit_program_create(const bx_wit_program_desc* desc, bx_wit_program** out) { return bx_wit_program_create_counted(desc, nullptr, 0, out); }

extern "C" const char* bx_acc_program_create(const bx_acc_program_desc* desc, bx_acc_program** out) try {
    if (!desc || !out) return "bx_acc_program_create: null argument";
    return bx::create(bx::acc_kind(), out, [&](bx_acc_program* p) { return bx::compile_acc(desc, p); });
} catch (...) {
    return "bx_acc_program_create: out of host memory";
}
