// wit_program_dev.hpp — a witness program loaded on a ctx: what wit_program.hip (load, unload, the interpreting kernel's launch) and
// program_gen.cpp (a generated kernel attached to it) share.  Host only.
#pragma once
#include "program_loaded.hpp"

struct bx_wit_program_dev {
    bx_ctx* ctx = nullptr;
    bx_wit_program_info info{};
    uint32_t n_fetch = 0, max_col[2] = {0, 0}, max_set = 0;
    size_t lds = 0;
    bx::DevBuf code, taps, consts;
    bx::GenKernel gen;  // bx_wit_program_attach_kernel; gen.digest is bx_wit_program_digest of the program this was loaded from
    // the multiplicity columns (wit_count.hip): the program's counts, where each one's sources start in the flat table and its bins
    // in the counters (sum of bins words), and the two on the device
    std::vector<bx::WitCount> counts;
    std::vector<size_t> count_src_off, count_bin_off;
    std::vector<uint32_t> count_flat;
    bx::DevBuf count_sources, count_bins;
    // the sorted columns (wit_sort.hip): the program's sorts, where each one's [sources | dests] start in the flat table, that table
    // on the device, and the work space (grown by the first run that needs more rows than sort_cap): the two (key, idx) pair buffers
    // in sort_pairs, the digit table and its chunk sums in sort_table
    std::vector<bx::WitSort> sorts;
    std::vector<size_t> sort_col_off;
    std::vector<uint32_t> sort_flat;
    bx::DevBuf sort_cols, sort_pairs, sort_table;
    size_t sort_cap = 0;
};

namespace bx {
// program_gen.cpp: launch the attached kernel: the caller (bx_wit_program_run) has checked the arguments
const char* wit_gen_launch(bx_ctx* c, bx_wit_program_dev* dev, uint32_t po2, bx_buf code, bx_buf data);
// wit_count.hip: upload the flat source table and allocate the counters (no-op without counts; the caller waits for the stream) ...
const char* wit_counts_load(bx_ctx* c, bx_wit_program_dev* dev, const bx_wit_program* prog);
// ... and per count clear, histogram, store on the ctx's stream: the caller (bx_wit_program_run) has checked the counts against the shape
const char* wit_counts_run(bx_ctx* c, bx_wit_program_dev* dev, uint32_t po2, bx_buf data);
// wit_sort.hip: upload the flat column table (no-op without sorts; the caller waits for the stream) ...
const char* wit_sorts_load(bx_ctx* c, bx_wit_program_dev* dev, const bx_wit_program* prog);
// ... and per sort pack, radix passes, gather on the ctx's stream (nothing at all without sorts): the caller (bx_wit_program_run) has
// checked the sorts against the shape
const char* wit_sorts_run(bx_ctx* c, bx_wit_program_dev* dev, uint32_t po2, bx_buf data);
}  // namespace bx
