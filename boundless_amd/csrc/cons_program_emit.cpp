// cons_program_emit.cpp — a compiled program as text (include/bx_program.h, "Generated kernels" and "Generated witness kernels", is
// the normative text): the digest of a constraint program and of a witness program, and the straight-line body that
// cons_program_gen.hpp / wit_program_gen.hpp frame into a gfx950 kernel or a host function.  Host only, plain C++, no ctx, no HIP:
// this translation unit compiles with g++ (tests/consgen_check.cpp and tests/witgen_check.cpp run it under sanitizers).
// The text is a pure function of the compiled program (cons_program.hpp): the stream, the constants, the taps, and n_globals,
// n_pows and ret_slot of a constraint program or the SET columns of a witness program.  Nothing else goes into it — no time, no
// path, no address.
// The two emitters share what follows first: Text, put_word / digest_words, the statements of the narrow opcodes, and the writer
// of one function or of segments.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "cons_program.hpp"
#include "cons_program_gen.hpp"
#include "sha256_suite.hpp"
#include "wit_program_gen.hpp"

namespace bx {
namespace {

void put_word(Sha256& h, uint32_t w) {
    const uint8_t b[4] = {(uint8_t)w, (uint8_t)(w >> 8), (uint8_t)(w >> 16), (uint8_t)(w >> 24)};
    h.update(b, 4);
}

// the stream, the constants and the taps, each led by its count: the part of a digest both kinds of program have
void put_tables(Sha256& h, const std::vector<uint32_t>& code, const std::vector<uint32_t>& consts, const std::vector<bx_cons_tap>& taps) {
    put_word(h, (uint32_t)code.size());
    for (uint32_t w : code) put_word(h, w);
    put_word(h, (uint32_t)consts.size());
    for (uint32_t w : consts) put_word(h, w);
    put_word(h, (uint32_t)taps.size());
    for (const bx_cons_tap& t : taps) put_word(h, t.group), put_word(h, t.col), put_word(h, t.back);
}

void digest_words(Sha256& h, uint32_t out[8]) {
    uint8_t d[32];
    h.finish(d);
    for (int k = 0; k < 8; ++k) out[k] = (uint32_t)d[4 * k] | (uint32_t)d[4 * k + 1] << 8 | (uint32_t)d[4 * k + 2] << 16 | (uint32_t)d[4 * k + 3] << 24;
}

void digest_of(const bx_cons_program* p, uint32_t out[8]) {
    Sha256 h;
    h.update((const uint8_t*)"bx-cons-program", 15);
    put_word(h, BX_CP_ABI);
    put_word(h, p->info.n_globals);
    put_word(h, p->n_pows);
    put_word(h, p->ret_slot);
    put_tables(h, p->code, p->consts, p->taps);
    digest_words(h, out);
}

// the global cells are NOT hashed: the kernel does not depend on them
void digest_of(const bx_wit_program* p, uint32_t out[8]) {
    Sha256 h;
    h.update((const uint8_t*)"bx-wit-program", 14);
    put_word(h, BX_WP_ABI);
    put_tables(h, p->code, p->consts, p->taps);
    put_word(h, (uint32_t)p->sets.size());
    for (uint32_t c : p->sets) put_word(h, c);
    digest_words(h, out);
}

struct Text {
    std::string s;
    void f(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        char line[256];
        va_list ap;
        va_start(ap, fmt);
        const int n = vsnprintf(line, sizeof line, fmt, ap);
        va_end(ap);
        s.append(line, n < 0 ? 0 : (size_t)n < sizeof line ? (size_t)n : sizeof line - 1);
    }
};

constexpr size_t CP_SEGMENT = 1024;  // instructions per function of the text (see write_functions)

struct Stmt {  // one instruction that does something
    std::string text;
    bool tap;
    uint32_t back;
};

const char* const group_fn[3] = {"code", "data", "accum"};

// the statements of the narrow opcodes both kinds of program have
void tap_stmt(Text& t, uint32_t d, const bx_cons_tap& tp) { t.f("    n%u = at.%s(%uu, r%u);\n", d, group_fn[tp.group], tp.col, tp.back); }
void const_stmt(Text& t, uint32_t d, uint32_t word) { t.f("    n%u = 0x%08xu;\n", d, word); }
void arith_bb_stmt(Text& t, uint32_t op, uint32_t d, uint32_t a, uint32_t b) {
    t.f("    n%u = %s(n%u, n%u);\n", d, op == CP_ADD_BB ? "fp_add" : (op == CP_SUB_BB ? "fp_sub" : "fp_mul"), a, b);
}

// what differs between the two texts around the statements
struct Frame {
    const char* lo;  // "bx_cp": the prefix of the text's own names
    const char* up;  // "BX_CP": ... and of the frame's macros
    uint32_t nn, nw;
    int ret_slot;  // the wide slot the body returns, or -1: the body returns nothing
};

// The statements as ONE function, every slot a local and nothing in memory; or, for a long program, as segments of CP_SEGMENT
// instructions, each a function of its own that is NOT inlined on the device.  The compiler's time grows faster than linearly with
// the size of one function (a 700-instruction body takes 11 s, an 8 000-instruction one did not finish in half an hour); segments
// keep it linear.  Between two segments the slot files go through a struct in memory, at fixed offsets: at most 128 words stored
// and loaded once per CP_SEGMENT instructions.
void write_functions(Text& t, const std::vector<Stmt>& stmts, const Frame& fr) {
    const uint32_t nn = fr.nn, nw = fr.nw;
    const char* const ret_type = fr.ret_slot < 0 ? "void" : "bx::Fp4";
    // the rows r<back> of the taps a function reads: once per distinct back
    const auto rows = [&](size_t from, size_t to) {
        std::set<uint32_t> backs;
        for (size_t k = from; k < to; ++k)
            if (stmts[k].tap) backs.insert(stmts[k].back);
        for (uint32_t b : backs) t.f("    const uint32_t r%u = at.row(%uu);\n", b, b);
    };
    if (stmts.size() <= CP_SEGMENT) {
        t.f("template <class A>\n%s_FN %s %s_body(const A& at) {\n    using namespace bx;\n", fr.up, ret_type, fr.lo);
        rows(0, stmts.size());
        for (uint32_t s = 0; s < nn; ++s) t.f("    uint32_t n%u = 0u;\n", s);
        for (uint32_t s = 0; s < nw; ++s) t.f("    Fp4 w%u = f4_zero();\n", s);
        for (const Stmt& st : stmts) t.s += st.text;
        if (fr.ret_slot >= 0) t.f("    return w%d;\n", fr.ret_slot);
        t.f("}\n\n%s_WRAPPERS\n", fr.up);
        return;
    }
    t.f("struct %s_slots {\n", fr.lo);
    for (uint32_t s = 0; s < nn; ++s) t.f("    uint32_t n%u;\n", s);
    for (uint32_t s = 0; s < nw; ++s) t.f("    bx::Fp4 w%u;\n", s);
    t.f("};\n\n");
    const size_t n_seg = (stmts.size() + CP_SEGMENT - 1) / CP_SEGMENT;
    for (size_t g = 0; g < n_seg; ++g) {
        const size_t from = g * CP_SEGMENT, to = from + CP_SEGMENT < stmts.size() ? from + CP_SEGMENT : stmts.size();
        t.f("template <class A>\n%s_SEG void %s_seg%zu(const A& at, %s_slots& s) {\n    using namespace bx;\n", fr.up, fr.lo, g, fr.lo);
        rows(from, to);
        for (uint32_t k = 0; k < nn; ++k) t.f("    uint32_t n%u = s.n%u;\n", k, k);
        for (uint32_t k = 0; k < nw; ++k) t.f("    Fp4 w%u = s.w%u;\n", k, k);
        for (size_t k = from; k < to; ++k) t.s += stmts[k].text;
        for (uint32_t k = 0; k < nn; ++k) t.f("    s.n%u = n%u;\n", k, k);
        for (uint32_t k = 0; k < nw; ++k) t.f("    s.w%u = w%u;\n", k, k);
        t.f("}\n\n");
    }
    t.f("template <class A>\n%s_FN %s %s_body(const A& at) {\n    %s_slots s = %s_slots();\n", fr.up, ret_type, fr.lo, fr.lo, fr.lo);
    for (size_t g = 0; g < n_seg; ++g) t.f("    %s_seg%zu(at, s);\n", fr.lo, g);
    if (fr.ret_slot >= 0) t.f("    return s.w%d;\n", fr.ret_slot);
    t.f("}\n\n%s_WRAPPERS\n", fr.up);
}

// a constraint program's body, one statement per instruction; false = the stream does not pass program_fits, and nothing is written
bool emit_text(const bx_cons_program* p, Text& out) {
    if (!program_fits(p)) return false;
    Text& t = out;
    const uint32_t nn = p->info.narrow, nw = p->info.wide, ng = p->info.n_globals;
    uint32_t dg[8];
    digest_of(p, dg);
    t.f("// generated by bx_cons_program_emit_hip: ABI %u, %u instructions, %u narrow and %u wide slots\n", BX_CP_ABI, p->info.instructions, nn, nw);
    t.f("#define BX_PLAIN_MAD 1\n#define BX_CP_DIGEST_WORDS 0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu\n", dg[0], dg[1], dg[2], dg[3], dg[4],
        dg[5], dg[6], dg[7]);
    t.f("#include \"cons_program_gen.hpp\"\n\n");
    std::vector<Stmt> stmts;  // in stream order
    for (size_t pc = 0; pc < p->code.size(); pc += 2) {
        Text t;  // this instruction's statement
        const uint32_t w0 = p->code[pc], w1 = p->code[pc + 1];
        const uint32_t op = w0 & 0xFFu, d = (w0 >> 8) & 0xFFu, a = (w0 >> 16) & 0xFFu, b = w0 >> 24, c = w1 & 0xFFu, imm = w1 >> 8;
        switch (op) {
        case CP_LD_B:
            if (imm < ng + 4) t.f("    n%u = at.scalar(%uu);\n", d, imm);
            else const_stmt(t, d, p->consts[imm - ng - 4]);
            break;
        case CP_LD_E: {
            const uint32_t* k = &p->consts[imm - ng - 4];
            t.f("    w%u = Fp4{{0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu}};\n", d, k[0], k[1], k[2], k[3]);
            break;
        }
        case CP_TAP: tap_stmt(t, d, p->taps[imm]); break;
        case CP_ADD_BB:
        case CP_SUB_BB:
        case CP_MUL_BB: arith_bb_stmt(t, op, d, a, b); break;
        case CP_ADD_EB:
        case CP_SUB_EB:
        case CP_MUL_EB: t.f("    w%u = %s(w%u, n%u);\n", d, op == CP_ADD_EB ? "cp_add_eb" : (op == CP_SUB_EB ? "cp_sub_eb" : "f4_scale"), a, b); break;
        case CP_SUB_BE: t.f("    w%u = cp_sub_be(n%u, w%u);\n", d, a, b); break;
        case CP_ADD_EE:
        case CP_SUB_EE:
        case CP_MUL_EE: t.f("    w%u = %s(w%u, w%u);\n", d, op == CP_ADD_EE ? "f4_add" : (op == CP_SUB_EE ? "f4_sub" : "f4_mul_lz"), a, b); break;
        case CP_ZERO: t.f("    w%u = f4_zero();\n", d); break;
        case CP_EQZ_B: t.f("    w%u = f4_add(w%u, f4_scale(at.power(%uu), n%u));\n", d, a, imm, b); break;
        case CP_EQZ_E: t.f("    w%u = f4_add(w%u, f4_mul_lz(at.power(%uu), w%u));\n", d, a, imm, b); break;
        case CP_COND_B: t.f("    w%u = f4_add(w%u, f4_scale(f4_mul_lz(at.power(%uu), w%u), n%u));\n", d, a, imm, c, b); break;
        case CP_COND_E: t.f("    w%u = f4_add(w%u, f4_mul_lz(f4_mul_lz(at.power(%uu), w%u), w%u));\n", d, a, imm, c, b); break;
        default: break;  // CP_NOP, the padding
        }
        if (!t.s.empty()) stmts.push_back(Stmt{t.s, op == CP_TAP, op == CP_TAP ? p->taps[imm].back : 0u});
    }
    write_functions(t, stmts, Frame{"bx_cp", "BX_CP", nn, nw, (int)p->ret_slot});
    return true;
}

// a witness program's body: the narrow opcodes and the store, nothing else; false as above
bool emit_text(const bx_wit_program* p, Text& out) {
    if (!program_fits(p)) return false;
    Text& t = out;
    const uint32_t nn = p->info.narrow;
    uint32_t dg[8];
    digest_of(p, dg);
    t.f("// generated by bx_wit_program_emit_hip: ABI %u, %u instructions, %u narrow slots, %zu derived columns\n", BX_WP_ABI, p->info.instructions, nn, p->sets.size());
    t.f("#define BX_WP_DIGEST_WORDS 0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu, 0x%08xu\n", dg[0], dg[1], dg[2], dg[3], dg[4], dg[5], dg[6], dg[7]);
    t.f("#include \"wit_program_gen.hpp\"\n\n");
    std::vector<Stmt> stmts;
    for (size_t pc = 0; pc < p->code.size(); pc += 2) {
        Text t;
        const uint32_t w0 = p->code[pc], w1 = p->code[pc + 1];
        const uint32_t op = w0 & 0xFFu, d = (w0 >> 8) & 0xFFu, a = (w0 >> 16) & 0xFFu, b = w0 >> 24, imm = w1 >> 8;
        switch (op) {
        case CP_LD_B: const_stmt(t, d, p->consts[imm]); break;  // `scal` is the constants alone
        case CP_TAP: tap_stmt(t, d, p->taps[imm]); break;
        case CP_ADD_BB:
        case CP_SUB_BB:
        case CP_MUL_BB: arith_bb_stmt(t, op, d, a, b); break;
        case CP_ST: t.f("    at.store(%uu, n%u);\n", imm, a); break;  // below max_set, which bx_wit_program_run holds against the data width
        default: break;  // CP_NOP, the padding
        }
        if (!t.s.empty()) stmts.push_back(Stmt{t.s, op == CP_TAP, op == CP_TAP ? p->taps[imm].back : 0u});
    }
    write_functions(t, stmts, Frame{"bx_wp", "BX_WP", nn, 0, -1});
    return true;
}

// the contract of both emit entry points: NULL buffer = size query, a short cap is refused with nothing written
const char* hand_out(const Text& t, char* buf, size_t cap, size_t* need, const char* short_msg) {
    *need = t.s.size() + 1;  // with the closing NUL
    if (!buf) return nullptr;
    if (cap < *need) return short_msg;
    memcpy(buf, t.s.c_str(), *need);
    return nullptr;
}

}  // namespace
}  // namespace bx

extern "C" const char* bx_cons_program_digest(const bx_cons_program* prog, uint32_t out[8]) try {
    if (!prog || !out) return "bx_cons_program_digest: null argument";
    bx::digest_of(prog, out);
    return nullptr;
} catch (...) {
    return "bx_cons_program_digest: out of host memory";
}

extern "C" const char* bx_cons_program_emit_hip(const bx_cons_program* prog, char* buf, size_t cap, size_t* need) try {
    if (!prog || !need) return "bx_cons_program_emit_hip: null argument";
    *need = 0;
    bx::Text t;
    if (!bx::emit_text(prog, t)) return "bx_cons_program_emit_hip: corrupt instruction stream";
    return bx::hand_out(t, buf, cap, need, "bx_cons_program_emit_hip: the buffer is shorter than the text (see *need)");
} catch (...) {
    return "bx_cons_program_emit_hip: out of host memory";
}

extern "C" const char* bx_wit_program_digest(const bx_wit_program* prog, uint32_t out[8]) try {
    if (!prog || !out) return "bx_wit_program_digest: null argument";
    bx::digest_of(prog, out);
    return nullptr;
} catch (...) {
    return "bx_wit_program_digest: out of host memory";
}

extern "C" const char* bx_wit_program_emit_hip(const bx_wit_program* prog, char* buf, size_t cap, size_t* need) try {
    if (!prog || !need) return "bx_wit_program_emit_hip: null argument";
    *need = 0;
    bx::Text t;
    if (!bx::emit_text(prog, t)) return "bx_wit_program_emit_hip: corrupt instruction stream";
    return bx::hand_out(t, buf, cap, need, "bx_wit_program_emit_hip: the buffer is shorter than the text (see *need)");
} catch (...) {
    return "bx_wit_program_emit_hip: out of host memory";
}
