// cons_program_dev.hpp — a constraint program loaded on a ctx: what cons_program.hip (load, unload, the interpreting kernel's launch)
// and program_gen.cpp (a generated kernel attached to it) share.  Host only.
#pragma once
#include "program_loaded.hpp"

struct bx_cons_program_dev {
    bx_ctx* ctx = nullptr;
    bx_cons_program_info info{};
    uint32_t n_pows = 1, ret_slot = 0, n_fetch = 0, max_col[3] = {0, 0, 0};
    size_t lds = 0;
    bx::DevBuf code, taps, scal, mixpows;
    bx::GenKernel gen;  // bx_cons_program_attach_kernel; gen.digest is bx_cons_program_digest of the program this was loaded from
};

namespace bx {
// program_gen.cpp: launch the attached kernel: the caller (bx_cons_program_eval_check) has checked the arguments and written `scal`
// and `mixpows`
const char* cons_gen_launch(bx_ctx* c, bx_cons_program_dev* dev, uint32_t po2, const uint32_t zinv[4], bx_buf check, bx_buf code_eval, bx_buf data_eval,
                            bx_buf accum_eval);
}  // namespace bx
