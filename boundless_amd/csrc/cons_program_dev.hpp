// cons_program_dev.hpp — a constraint program loaded on a ctx: what cons_program.hip (load, unload, the interpreting kernel's launch)
// and cons_program_gen.cpp (a generated kernel attached to it) share.  Host only.
#pragma once
#include "cons_program.hpp"
#include "ctx.hpp"

struct bx_cons_program_dev {
    bx_ctx* ctx = nullptr;
    bx_cons_program_info info{};
    uint32_t n_pows = 1, ret_slot = 0, n_fetch = 0, max_col[3] = {0, 0, 0};
    size_t lds = 0;
    bx::DevBuf code, taps, scal, mixpows;
    // the generated kernel (bx_cons_program_attach_kernel): none unless gen_fn is set
    uint32_t digest[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // bx_cons_program_digest of the program this was loaded from
    hipModule_t gen_module = nullptr;
    hipFunction_t gen_fn = nullptr;
};

namespace bx {
// cons_program_gen.cpp, shared with wit_program_gen.cpp: does `image` start with the ELF magic or "__CLANG_OFFLOAD_BUNDLE__"; and a
// device symbol of `m` copied back (false = the module has no such symbol of that size)
bool has_code_object_magic(const void* image, size_t len);
bool read_symbol(bx_ctx* c, hipModule_t m, const char* name, uint32_t* out, size_t words);
// cons_program_gen.cpp: unload what is attached (no-op when nothing is; the caller has drained the stream)
void cons_gen_release(bx_cons_program_dev* dev);
// ... and launch it: the caller (bx_cons_program_eval_check) has checked the arguments and written `scal` and `mixpows`
const char* cons_gen_launch(bx_ctx* c, bx_cons_program_dev* dev, uint32_t po2, const uint32_t zinv[4], bx_buf check, bx_buf code_eval, bx_buf data_eval,
                            bx_buf accum_eval);
}  // namespace bx
