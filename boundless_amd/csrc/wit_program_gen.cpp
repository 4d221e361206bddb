// wit_program_gen.cpp — a generated derive kernel on a loaded witness program (include/bx_program.h, "Generated witness kernels", is
// the normative text; wit_program_gen.hpp the kernel's frame and ABI): attach, detach and launch, as cons_program_gen.cpp does them
// for constraint programs, in the same order of checks.  Host only: the kernel arrives as a code object built off line
// (boundless_amd/consgen.py --witness) and is loaded with the HIP module API; nothing is compiled at run time.
// What reaches HIP: an image with a code object's magic, and only that.  What reaches a launch: a module whose bx_wp_abi is
// BX_WP_ABI and whose bx_wp_digest is the digest of the program it is attached to.
#include <string.h>

#include "cons_program_dev.hpp"
#include "wit_program_dev.hpp"
#include "wit_program_gen.hpp"

namespace bx {

void wit_gen_release(bx_wit_program_dev* dev) {
    if (dev->gen_module) (void)hipModuleUnload(dev->gen_module);
    dev->gen_module = nullptr;
    dev->gen_fn = nullptr;
}

const char* wit_gen_launch(bx_ctx* c, bx_wit_program_dev* dev, uint32_t po2, bx_buf code, bx_buf data) {
    const size_t n = (size_t)1 << po2;
    bx_wp_gen_args a;
    a.data = (uint32_t*)data.dptr;
    a.code = (const uint32_t*)code.dptr;
    a.n = (uint32_t)n;
    a.po2 = po2;
    void* params[] = {&a};
    // every tap is read once, every derived column written once; a name of its own, so that a profile tells the two executors apart
    OpScope op(c, "wit_program_run_gen", 4.0 * (double)n * ((double)dev->info.taps + (double)dev->info.sets));
    BX_HIP(c, hipModuleLaunchKernel(dev->gen_fn, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, c->stream, params, nullptr));
    return nullptr;
}

}  // namespace bx

extern "C" const char* bx_wit_program_attach_kernel(bx_wit_program_dev* dev, const void* image, size_t len) try {
    using namespace bx;
    if (!dev || !dev->ctx) return "bx_wit_program_attach_kernel: null program";
    bx_ctx* c = dev->ctx;
    BX_REQUIRE(c, image != nullptr, "bx_wit_program_attach_kernel: null image");
    BX_REQUIRE(c, dev->gen_fn == nullptr, "bx_wit_program_attach_kernel: a kernel is already attached (detach it first)");
    BX_REQUIRE(c, has_code_object_magic(image, len), "bx_wit_program_attach_kernel: the image is neither an ELF code object nor a clang offload bundle");
    BX_ENTER(c);
    hipModule_t m = nullptr;
    if (hipError_t e = hipModuleLoadData(&m, image)) {
        (void)hipGetLastError();
        snprintf(c->err, sizeof c->err, "bx_wit_program_attach_kernel: the code object does not load on this device (%s)", hipGetErrorString(e));
        return c->err;
    }
    const char* refusal = nullptr;
    hipFunction_t fn = nullptr;
    uint32_t abi = 0, digest[8];
    if (hipModuleGetFunction(&fn, m, "bx_wp_run") != hipSuccess) {
        (void)hipGetLastError();
        refusal = "bx_wit_program_attach_kernel: the code object has no kernel bx_wp_run";
    } else if (!read_symbol(c, m, "bx_wp_abi", &abi, 1) || !read_symbol(c, m, "bx_wp_digest", digest, 8)) {
        refusal = "bx_wit_program_attach_kernel: the code object lacks the symbol bx_wp_abi or bx_wp_digest";
    } else if (abi != BX_WP_ABI) {
        snprintf(c->err, sizeof c->err, "bx_wit_program_attach_kernel: the kernel was built for ABI %u, this library launches ABI %u", abi, BX_WP_ABI);
        refusal = c->err;
    } else if (memcmp(digest, dev->digest, sizeof digest) != 0) {
        snprintf(c->err, sizeof c->err, "bx_wit_program_attach_kernel: digest mismatch: the kernel was generated from another program (%08x..., loaded %08x...)", digest[0],
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
} BX_ABI_CATCH(dev ? dev->ctx : nullptr, "bx_wit_program_attach_kernel")

extern "C" const char* bx_wit_program_detach_kernel(bx_wit_program_dev* dev) try {
    using namespace bx;
    if (!dev || !dev->ctx) return "bx_wit_program_detach_kernel: null program";
    bx_ctx* c = dev->ctx;
    BX_REQUIRE(c, dev->gen_fn != nullptr, "bx_wit_program_detach_kernel: no kernel is attached");
    BX_ENTER(c);
    BX_HIP(c, stream_wait(c));  // a launch may still run it
    wit_gen_release(dev);
    return nullptr;
} BX_ABI_CATCH(dev ? dev->ctx : nullptr, "bx_wit_program_detach_kernel")

extern "C" int bx_wit_program_kernel_attached(const bx_wit_program_dev* dev) { return dev && dev->gen_fn ? 1 : 0; }
