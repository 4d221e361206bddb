// cons_program_gen.cpp — a generated eval_check kernel on a loaded constraint program (include/bx_program.h, "Generated kernels", is
// the normative text; cons_program_gen.hpp the kernel's frame and ABI): attach, detach and launch.  Host only: the kernel arrives as a
// code object built off line (boundless_amd/consgen.py) and is loaded with the HIP module API; nothing is compiled at run time.
// What reaches HIP: an image with a code object's magic, and only that.  What reaches a launch: a module whose bx_cp_abi is
// BX_CP_ABI and whose bx_cp_digest is the digest of the program it is attached to.
#include <string.h>

#include "cons_program_dev.hpp"
#include "cons_program_gen.hpp"

namespace bx {

bool has_code_object_magic(const void* image, size_t len) {
    static const char elf[4] = {0x7f, 'E', 'L', 'F'};
    static const char bundle[] = "__CLANG_OFFLOAD_BUNDLE__";
    return (len >= sizeof elf && memcmp(image, elf, sizeof elf) == 0) || (len >= sizeof bundle - 1 && memcmp(image, bundle, sizeof bundle - 1) == 0);
}

// a device symbol of `m` copied back; false = the module has no such symbol of that size
bool read_symbol(bx_ctx* c, hipModule_t m, const char* name, uint32_t* out, size_t words) {
    hipDeviceptr_t p = nullptr;
    size_t bytes = 0;
    if (hipModuleGetGlobal(&p, &bytes, m, name) != hipSuccess || bytes != 4 * words) {
        (void)hipGetLastError();
        return false;
    }
    if (hipMemcpyAsync(out, p, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess || stream_wait(c) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}

void cons_gen_release(bx_cons_program_dev* dev) {
    if (dev->gen_module) (void)hipModuleUnload(dev->gen_module);
    dev->gen_module = nullptr;
    dev->gen_fn = nullptr;
}

const char* cons_gen_launch(bx_ctx* c, bx_cons_program_dev* dev, uint32_t po2, const uint32_t zinv[4], bx_buf check, bx_buf code_eval, bx_buf data_eval,
                            bx_buf accum_eval) {
    const size_t dom = (size_t)4 << po2;
    bx_cp_gen_args a;
    a.check = (uint32_t*)check.dptr;
    a.ecode = (const uint32_t*)code_eval.dptr;
    a.edata = (const uint32_t*)data_eval.dptr;
    a.eacc = (const uint32_t*)accum_eval.dptr;
    a.scal = (const uint32_t*)dev->scal.b.dptr;
    a.mixpows = (const uint32_t*)dev->mixpows.b.dptr;
    for (int k = 0; k < 4; ++k) a.zinv[k] = zinv[k];
    a.dom = (uint32_t)dom;
    a.po2 = po2;
    void* params[] = {&a};
    // every tap is read once, four planes are written; a name of its own, so that a profile tells the two executors apart
    OpScope op(c, "cons_program_eval_check_gen", 4.0 * (double)dom * ((double)dev->info.taps + 4.0));
    BX_HIP(c, hipModuleLaunchKernel(dev->gen_fn, (unsigned)((dom + 255) / 256), 1, 1, 256, 1, 1, 0, c->stream, params, nullptr));
    return nullptr;
}

}  // namespace bx

extern "C" const char* bx_cons_program_attach_kernel(bx_cons_program_dev* dev, const void* image, size_t len) try {
    using namespace bx;
    if (!dev || !dev->ctx) return "bx_cons_program_attach_kernel: null program";
    bx_ctx* c = dev->ctx;
    BX_REQUIRE(c, image != nullptr, "bx_cons_program_attach_kernel: null image");
    BX_REQUIRE(c, dev->gen_fn == nullptr, "bx_cons_program_attach_kernel: a kernel is already attached (detach it first)");
    BX_REQUIRE(c, has_code_object_magic(image, len), "bx_cons_program_attach_kernel: the image is neither an ELF code object nor a clang offload bundle");
    BX_ENTER(c);
    hipModule_t m = nullptr;
    if (hipError_t e = hipModuleLoadData(&m, image)) {
        (void)hipGetLastError();
        snprintf(c->err, sizeof c->err, "bx_cons_program_attach_kernel: the code object does not load on this device (%s)", hipGetErrorString(e));
        return c->err;
    }
    const char* refusal = nullptr;
    hipFunction_t fn = nullptr;
    uint32_t abi = 0, digest[8];
    if (hipModuleGetFunction(&fn, m, "bx_cp_eval") != hipSuccess) {
        (void)hipGetLastError();
        refusal = "bx_cons_program_attach_kernel: the code object has no kernel bx_cp_eval";
    } else if (!read_symbol(c, m, "bx_cp_abi", &abi, 1) || !read_symbol(c, m, "bx_cp_digest", digest, 8)) {
        refusal = "bx_cons_program_attach_kernel: the code object lacks the symbol bx_cp_abi or bx_cp_digest";
    } else if (abi != BX_CP_ABI) {
        snprintf(c->err, sizeof c->err, "bx_cons_program_attach_kernel: the kernel was built for ABI %u, this library launches ABI %u", abi, BX_CP_ABI);
        refusal = c->err;
    } else if (memcmp(digest, dev->digest, sizeof digest) != 0) {
        snprintf(c->err, sizeof c->err, "bx_cons_program_attach_kernel: digest mismatch: the kernel was generated from another program (%08x..., loaded %08x...)", digest[0],
                 dev->digest[0]);
        refusal = c->err;
    }
    if (refusal) {
        (void)hipModuleUnload(m);
        return refusal == c->err ? refusal : set_msg(c, refusal);
    }
    dev->gen_module = m;
    dev->gen_fn = fn;
    return nullptr;
} BX_ABI_CATCH(dev ? dev->ctx : nullptr, "bx_cons_program_attach_kernel")

extern "C" const char* bx_cons_program_detach_kernel(bx_cons_program_dev* dev) try {
    using namespace bx;
    if (!dev || !dev->ctx) return "bx_cons_program_detach_kernel: null program";
    bx_ctx* c = dev->ctx;
    BX_REQUIRE(c, dev->gen_fn != nullptr, "bx_cons_program_detach_kernel: no kernel is attached");
    BX_ENTER(c);
    BX_HIP(c, stream_wait(c));  // a launch may still run it
    cons_gen_release(dev);
    return nullptr;
} BX_ABI_CATCH(dev ? dev->ctx : nullptr, "bx_cons_program_detach_kernel")

extern "C" int bx_cons_program_kernel_attached(const bx_cons_program_dev* dev) { return dev && dev->gen_fn ? 1 : 0; }
