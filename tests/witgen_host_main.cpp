// witgen_host_main.cpp — runs ONE generated witness-program body on the CPU (tests/test_witgen_cpu.py): the text
// bx_wit_program_emit_hip wrote is included below as bx_wp_generated.inc, compiled by g++ under -fsanitize=address,undefined through
// the host wrapper of csrc/wit_program_gen.hpp, and linked with csrc/program_compile.cpp and csrc/cons_program_host.cpp.
//
//     witgen_host CASE.bin DATA.bin [CASE.bin DATA.bin ...]
//
// CASE.bin, 32-bit little-endian words: po2, w_code, w_data, n_steps, n_taps, n_cells; the steps (op a b c d), the taps
// (group col back) and the cells (global col row); the code group and the data group, N x width column-major, Montgomery words.
// DATA.bin receives the data group after bx_wp_run_host (Python compares it with the numpy reference).  Here it must equal, word for
// word, what bx_wit_program_run_host makes of the same description and columns, and the text's digest must be the description's.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bx_program.h"
#include "bx_wp_generated.inc"

static int one(const char* case_path, const char* out_path) {
    std::vector<uint32_t> in;
    {
        FILE* f = fopen(case_path, "rb");
        if (!f) return 2;
        uint32_t buf[4096];
        size_t n;
        while ((n = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + n);
        fclose(f);
    }
    if (in.size() < 6) return 2;
    const uint32_t po2 = in[0], w_code = in[1], w_data = in[2], n_steps = in[3], n_taps = in[4], n_cells = in[5];
    if (po2 < 1 || po2 > 16) return 2;
    const uint32_t n = 1u << po2;
    const size_t want = 6 + 5 * (size_t)n_steps + 3 * (size_t)n_taps + 3 * (size_t)n_cells + (size_t)n * (w_code + w_data);
    if (in.size() != want) {
        printf("%s has %zu words, its header says %zu\n", case_path, in.size(), want);
        return 2;
    }
    const uint32_t* p = in.data() + 6;
    std::vector<bx_cons_step> steps(n_steps);
    for (bx_cons_step& s : steps) s = bx_cons_step{p[0], p[1], p[2], p[3], p[4]}, p += 5;
    std::vector<bx_cons_tap> taps(n_taps);
    for (bx_cons_tap& t : taps) t = bx_cons_tap{p[0], p[1], p[2]}, p += 3;
    std::vector<bx_wit_global_cell> cells(n_cells);
    for (bx_wit_global_cell& g : cells) g = bx_wit_global_cell{p[0], p[1], p[2]}, p += 3;
    const std::vector<uint32_t> code(p, p + (size_t)n * w_code), data(p + (size_t)n * w_code, p + (size_t)n * (w_code + w_data));

    bx_wit_program_desc d{steps.data(), steps.size(), taps.data(), taps.size(), cells.data(), cells.size()};
    bx_wit_program* prog = nullptr;
    if (const char* e = bx_wit_program_create(&d, &prog)) {
        printf("create: %s\n", e);
        return 1;
    }
    uint32_t dg[8];
    bx_wit_program_digest(prog, dg);
    if (memcmp(dg, bx_wp_digest, 32) != 0 || bx_wp_abi != 1u) {
        printf("the generated text carries another program's digest\n");
        return 1;
    }
    std::vector<uint32_t> host = data, gen = data;
    if (const char* e = bx_wit_program_run_host(prog, po2, code.data(), w_code, host.data(), w_data)) {  // also: every column is within the widths
        printf("run_host: %s\n", e);
        return 1;
    }
    bx_wp_gen_args a;
    a.data = gen.data();
    a.code = code.data();
    a.n = n, a.po2 = po2;
    bx_wp_run_host(a);
    for (size_t k = 0; k < gen.size(); ++k)
        if (gen[k] != host[k]) {
            printf("%s: data[%zu][%zu] is %u by the generated body, %u by bx_wit_program_run_host\n", case_path, k / n, k % n, gen[k], host[k]);
            return 1;
        }
    bx_wit_program_destroy(prog);
    FILE* f = fopen(out_path, "wb");
    if (!f || fwrite(gen.data(), 4, gen.size(), f) != gen.size()) return 2;
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3 || argc % 2 == 0) return 2;
    for (int k = 1; k + 1 < argc; k += 2)
        if (int rc = one(argv[k], argv[k + 1])) return rc;
    printf("witgen_host ok: %d cases\n", (argc - 1) / 2);
    return 0;
}
