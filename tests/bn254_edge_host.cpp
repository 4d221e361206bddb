// bn254_edge_host.cpp — the host build of the BN254 edge-operand op table (tests/bn254_edge_ops.hpp): reads an operand file, writes
// a result file.  Stand-alone (its own main), so it also runs under -fsanitize=address,undefined as an ordinary child process.
//   operand file: u32 words [MAGIC, family, count, words per record] then count records;  result file: count result rows.
//   usage: bn254_edge_host <operands> <results>
#include <stdio.h>

#include <vector>

#include "bn254_edge_ops.hpp"

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <operands> <results>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t hdr[4];
    if (fread(hdr, 4, 4, f) != 4 || hdr[0] != 0x45444742u || hdr[1] >= bn_edge::N_FAMILIES || hdr[3] != bn_edge::words_in(hdr[1])) {
        fprintf(stderr, "%s: bad header\n", argv[1]);
        return 2;
    }
    const size_t count = hdr[2], nin = hdr[3], nout = bn_edge::words_out(hdr[1]);
    std::vector<uint32_t> in(count * nin), out(count * nout);
    if (fread(in.data(), 4, in.size(), f) != in.size() || fgetc(f) != EOF) {
        fprintf(stderr, "%s: length does not match its header\n", argv[1]);
        return 2;
    }
    fclose(f);
    for (size_t i = 0; i < count; i++) bn_edge::apply(hdr[1], in.data() + i * nin, out.data() + i * nout);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    return 0;
}
