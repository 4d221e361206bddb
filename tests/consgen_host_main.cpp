// consgen_host_main.cpp — runs ONE generated constraint-program body on the CPU (tests/test_consgen_cpu.py): the text
// bx_cons_program_emit_hip wrote is included below as bx_cp_generated.inc, compiled by g++ under -fsanitize=address,undefined through
// the host wrapper of csrc/cons_program_gen.hpp, and linked with csrc/program_compile.cpp and csrc/cons_program_host.cpp.
//
//     consgen_host CASE.bin PLANES.bin
//
// CASE.bin, 32-bit little-endian words: po2, the three widths, n_globals, ret, n_steps, n_taps; the steps (op a b c d) and the taps
// (group col back); globals, mix (4), poly_mix (4), zinv (4) as Montgomery words; the three evaluation groups, 4N x width column-major.
// PLANES.bin receives the four check planes over the whole domain (Python compares them with the reference).  Here, at every domain
// point, the body's value must equal bx_cons_program_constraints_at of the same description fed the base tap values as (v, 0, 0, 0):
// the embedding of the base field is a ring map, so the verifier's executor and the prover's generated code must agree.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bx_program.h"
#include "bx_cp_generated.inc"

struct Reader {
    const uint32_t* group[3];
    uint32_t dom, i;
};
static const char* tap_at(const void* ctx, int group, uint32_t col, int back, uint32_t out[4]) {
    const Reader* r = (const Reader*)ctx;
    out[0] = r->group[group][(size_t)col * r->dom + ((r->i - 4u * (uint32_t)back) & (r->dom - 1u))];
    out[1] = out[2] = out[3] = 0u;
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::vector<uint32_t> in;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        uint32_t buf[4096];
        size_t n;
        while ((n = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + n);
        fclose(f);
    }
    if (in.size() < 8) return 2;
    const uint32_t po2 = in[0], w[3] = {in[1], in[2], in[3]}, ng = in[4], ret = in[5], n_steps = in[6], n_taps = in[7];
    const uint32_t dom = 4u << po2;
    const size_t want = 8 + 5 * (size_t)n_steps + 3 * (size_t)n_taps + ng + 12 + (size_t)dom * (w[0] + w[1] + w[2]);
    if (in.size() != want) {
        printf("the case file has %zu words, its header says %zu\n", in.size(), want);
        return 2;
    }
    const uint32_t* p = in.data() + 8;
    std::vector<bx_cons_step> steps(n_steps);
    for (bx_cons_step& s : steps) s = bx_cons_step{p[0], p[1], p[2], p[3], p[4]}, p += 5;
    std::vector<bx_cons_tap> taps(n_taps);
    for (bx_cons_tap& t : taps) t = bx_cons_tap{p[0], p[1], p[2]}, p += 3;
    const uint32_t* globals = p;
    const uint32_t* mix = p + ng;
    const uint32_t* poly_mix = mix + 4;
    const uint32_t* zinv = poly_mix + 4;
    const uint32_t* ev[3] = {zinv + 4, zinv + 4 + (size_t)dom * w[0], zinv + 4 + (size_t)dom * (w[0] + w[1])};

    bx_cons_program_desc d{steps.data(), steps.size(), taps.data(), taps.size(), ng, ret};
    bx_cons_program* prog = nullptr;
    if (const char* e = bx_cons_program_create(&d, &prog)) {
        printf("create: %s\n", e);
        return 1;
    }
    uint32_t dg[8];
    bx_cons_program_digest(prog, dg);
    if (memcmp(dg, bx_cp_digest, 32) != 0 || bx_cp_abi != 1u) {
        printf("the generated text carries another program's digest\n");
        return 1;
    }
    bx_cons_program_info info;
    bx_cons_program_info_get(prog, &info);
    for (const bx_cons_tap& t : taps)
        if (t.col >= w[t.group]) {
            printf("tap column %u of group %u is outside the case's widths\n", t.col, t.group);
            return 1;
        }
    // the canonical mix powers (the first half of mix_power_table), exactly as many as the program can name
    std::vector<uint32_t> pows(4 * ((size_t)info.constraints + 1));
    bx::Fp4 pw = bx::f4_one();
    const bx::Fp4 pm{{poly_mix[0], poly_mix[1], poly_mix[2], poly_mix[3]}};
    for (uint32_t e = 0; e <= info.constraints; ++e) {
        memcpy(&pows[4 * (size_t)e], pw.c, 16);
        pw = bx::f4_mul(pw, pm);
    }
    std::vector<uint32_t> scal(ng + 4), planes(4 * (size_t)dom, 0xFFFFFFFFu);
    for (uint32_t k = 0; k < ng; ++k) scal[k] = globals[k];
    for (uint32_t k = 0; k < 4; ++k) scal[ng + k] = mix[k];
    bx_cp_gen_args a;
    a.check = planes.data();
    a.ecode = ev[0], a.edata = ev[1], a.eacc = ev[2];
    a.scal = scal.data();
    a.mixpows = pows.data();
    for (int k = 0; k < 4; ++k) a.zinv[k] = zinv[k];
    a.dom = dom, a.po2 = po2;
    bx_cp_eval_host(a);

    Reader rd{{ev[0], ev[1], ev[2]}, dom, 0};
    const bx_tap_reader reader{&rd, tap_at};
    for (uint32_t i = 0; i < dom; ++i) {
        rd.i = i;
        uint32_t at[4];
        if (const char* e = bx_cons_program_constraints_at(prog, &reader, poly_mix, mix, globals, at)) {
            printf("constraints_at: %s\n", e);
            return 1;
        }
        const bx::Fp4 got = bx_cp_body_at(a, i);
        if (memcmp(got.c, at, 16) != 0) {
            printf("point %u: the generated body gives (%u %u %u %u), constraints_at (%u %u %u %u)\n", i, got.c[0], got.c[1], got.c[2], got.c[3], at[0], at[1], at[2], at[3]);
            return 1;
        }
    }
    bx_cons_program_destroy(prog);
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(planes.data(), 4, planes.size(), f) != planes.size()) return 2;
    fclose(f);
    printf("consgen_host ok: %u points\n", dom);
    return 0;
}
