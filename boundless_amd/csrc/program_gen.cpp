// program_gen.cpp — a generated kernel on a loaded constraint or witness program (include/bx_program.h, "Generated kernels" and
// "Generated witness kernels", is the normative text; cons_program_gen.hpp and wit_program_gen.hpp the kernels' frames and ABIs):
// ONE attach, detach and release over the GenKernel a loaded program embeds (program_loaded.hpp), told apart by a GenKind, and each
// kind's launch.  Host only: a kernel arrives as a code object built off line (boundless_amd/consgen.py) and is loaded with the HIP
// module API; nothing is compiled at run time.
// What reaches HIP: an image with a code object's magic, and only that.  What reaches a launch: a module whose ABI symbol holds the
// number this library launches and whose digest symbol holds the digest of the program it is attached to.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "cons_program_dev.hpp"
#include "cons_program_gen.hpp"
#include "wit_program_dev.hpp"
#include "wit_program_gen.hpp"

namespace bx {
namespace {

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

const char* says(bx_ctx* c, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
const char* says(bx_ctx* c, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof c->err, fmt, ap);
    va_end(ap);
    return c->err;
}

// functions, not objects: a namespace-scope constant would be emitted for the device too
GenKind cons_gen_kind() { return GenKind{"bx_cons_program", "bx_cp_eval", "bx_cp_abi", "bx_cp_digest", BX_CP_ABI}; }
GenKind wit_gen_kind() { return GenKind{"bx_wit_program", "bx_wp_run", "bx_wp_abi", "bx_wp_digest", BX_WP_ABI}; }

}  // namespace

void gen_release(GenKernel& g) {
    if (g.module) (void)hipModuleUnload(g.module);
    g.module = nullptr;
    g.fn = nullptr;
}

const char* gen_attach(bx_ctx* c, GenKernel& g, const GenKind& k, const void* image, size_t len) {
    if (!image) return says(c, "%s_attach_kernel: null image", k.who);
    if (g.fn) return says(c, "%s_attach_kernel: a kernel is already attached (detach it first)", k.who);
    if (!has_code_object_magic(image, len)) return says(c, "%s_attach_kernel: the image is neither an ELF code object nor a clang offload bundle", k.who);
    BX_ENTER(c);
    hipModule_t m = nullptr;
    if (hipError_t e = hipModuleLoadData(&m, image)) {
        (void)hipGetLastError();
        return says(c, "%s_attach_kernel: the code object does not load on this device (%s)", k.who, hipGetErrorString(e));
    }
    const char* refusal = nullptr;
    hipFunction_t fn = nullptr;
    uint32_t abi = 0, digest[8];
    if (hipModuleGetFunction(&fn, m, k.kernel) != hipSuccess) {
        (void)hipGetLastError();
        refusal = says(c, "%s_attach_kernel: the code object has no kernel %s", k.who, k.kernel);
    } else if (!read_symbol(c, m, k.abi_symbol, &abi, 1) || !read_symbol(c, m, k.digest_symbol, digest, 8)) {
        refusal = says(c, "%s_attach_kernel: the code object lacks the symbol %s or %s", k.who, k.abi_symbol, k.digest_symbol);
    } else if (abi != k.abi) {
        refusal = says(c, "%s_attach_kernel: the kernel was built for ABI %u, this library launches ABI %u", k.who, abi, k.abi);
    } else if (memcmp(digest, g.digest, sizeof digest) != 0) {
        refusal = says(c, "%s_attach_kernel: digest mismatch: the kernel was generated from another program (%08x..., loaded %08x...)", k.who, digest[0], g.digest[0]);
    }
    if (refusal) {
        (void)hipModuleUnload(m);
        return refusal;
    }
    g.module = m;
    g.fn = fn;
    return nullptr;
}

const char* gen_detach(bx_ctx* c, GenKernel& g, const GenKind& k) {
    if (!g.fn) return says(c, "%s_detach_kernel: no kernel is attached", k.who);
    BX_ENTER(c);
    BX_HIP(c, stream_wait(c));  // a launch may still run it
    gen_release(g);
    return nullptr;
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
    BX_HIP(c, hipModuleLaunchKernel(dev->gen.fn, (unsigned)((dom + 255) / 256), 1, 1, 256, 1, 1, 0, c->stream, params, nullptr));
    return nullptr;
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
    BX_HIP(c, hipModuleLaunchKernel(dev->gen.fn, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, c->stream, params, nullptr));
    return nullptr;
}

}  // namespace bx

extern "C" const char* bx_cons_program_attach_kernel(bx_cons_program_dev* dev, const void* image, size_t len) try {
    if (!dev || !dev->ctx) return "bx_cons_program_attach_kernel: null program";
    return bx::gen_attach(dev->ctx, dev->gen, bx::cons_gen_kind(), image, len);
} BX_ABI_CATCH(dev ? dev->ctx : nullptr, "bx_cons_program_attach_kernel")

extern "C" const char* bx_cons_program_detach_kernel(bx_cons_program_dev* dev) try {
    if (!dev || !dev->ctx) return "bx_cons_program_detach_kernel: null program";
    return bx::gen_detach(dev->ctx, dev->gen, bx::cons_gen_kind());
} BX_ABI_CATCH(dev ? dev->ctx : nullptr, "bx_cons_program_detach_kernel")

extern "C" int bx_cons_program_kernel_attached(const bx_cons_program_dev* dev) { return dev && dev->gen.fn ? 1 : 0; }

extern "C" const char* bx_wit_program_attach_kernel(bx_wit_program_dev* dev, const void* image, size_t len) try {
    if (!dev || !dev->ctx) return "bx_wit_program_attach_kernel: null program";
    return bx::gen_attach(dev->ctx, dev->gen, bx::wit_gen_kind(), image, len);
} BX_ABI_CATCH(dev ? dev->ctx : nullptr, "bx_wit_program_attach_kernel")

extern "C" const char* bx_wit_program_detach_kernel(bx_wit_program_dev* dev) try {
    if (!dev || !dev->ctx) return "bx_wit_program_detach_kernel: null program";
    return bx::gen_detach(dev->ctx, dev->gen, bx::wit_gen_kind());
} BX_ABI_CATCH(dev ? dev->ctx : nullptr, "bx_wit_program_detach_kernel")

extern "C" int bx_wit_program_kernel_attached(const bx_wit_program_dev* dev) { return dev && dev->gen.fn ? 1 : 0; }
