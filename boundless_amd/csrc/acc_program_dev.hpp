// acc_program_dev.hpp — an accumulate program loaded on a ctx: what acc_program.hip (load, unload, keep, run) owns and what a
// generated kernel attached to it would share, as cons_program_dev.hpp and wit_program_dev.hpp are.  Host only.
#pragma once
#include "program_loaded.hpp"

struct bx_acc_program_dev {
    bx_ctx* ctx = nullptr;
    bx_acc_program_info info{};
    uint32_t ratios = 0;  // R of the compiled program: run_ext holds S + R sequences
    uint32_t n_fetch = 0;
    size_t lds = 0;
    std::vector<bx_cons_tap> kept_cols;  // host copy of the kept list: the width checks of keep
    // code: the stream; taps: (kept index, back) per tap; kept: (group, col) per kept column; scal: [globals | mix | constants]
    bx::DevBuf code, taps, kept, scal;
};
