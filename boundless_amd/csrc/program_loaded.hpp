// program_loaded.hpp — what a program of any kind LOADED on a ctx shares (cons_program.hip, wit_program.hip, acc_program.hip and
// program_gen.cpp): the registry of what bx_free still has to release, the upload of the tables, the LDS attribute of an interpreting
// kernel, and a generated kernel attached to a loaded program.  Host only.
#pragma once
#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "cons_program.hpp"
#include "ctx.hpp"

namespace bx {

// The loaded programs of one kind, per ctx.  A handle is looked up BY ADDRESS and never read: one that was unloaded twice, or whose
// ctx was freed, names freed memory.
template <class Dev>
class LoadedPrograms {
    std::mutex mu;
    std::map<bx_ctx*, std::set<Dev*>> by_ctx;

public:
    void insert(bx_ctx* c, Dev* d) {
        std::lock_guard<std::mutex> g(mu);
        by_ctx[c].insert(d);
    }
    // takes `d` out and returns the ctx it was loaded on; NULL = not a loaded program
    bx_ctx* take(Dev* d) {
        std::lock_guard<std::mutex> g(mu);
        for (auto it = by_ctx.begin(); it != by_ctx.end(); ++it)
            if (it->second.erase(d)) {
                bx_ctx* c = it->first;
                if (it->second.empty()) by_ctx.erase(it);
                return c;
            }
        return nullptr;
    }
    // takes out everything still loaded on `c`
    std::set<Dev*> take_all(bx_ctx* c) {
        std::set<Dev*> ds;
        std::lock_guard<std::mutex> g(mu);
        auto it = by_ctx.find(c);
        if (it == by_ctx.end()) return ds;
        ds.swap(it->second);
        by_ctx.erase(it);
        return ds;
    }
};

// The upload every load ends with, on the ctx's stream: the instruction stream, the tap list as two words per tap (`pack(words, t, tap)`
// writes them: each kind's kernel reads its own form), and `scal` with the constants at `consts_at` and zeros in front of them (the
// words a launch writes).  Allocates the three buffers (never empty) before the first copy, and WAITS for the stream before its
// host vectors go away.  A load with a further table uploads it afterwards, with a wait of its own.
template <class Pack>
const char* upload_program(bx_ctx* c, DevBuf& code, DevBuf& taps, DevBuf& scal, const std::vector<uint32_t>& stream, const std::vector<bx_cons_tap>& tap_list, Pack pack,
                           const std::vector<uint32_t>& consts, size_t consts_at) {
    std::vector<uint32_t> tapw(2 * tap_list.size()), scalw(consts_at + consts.size(), 0u);
    for (size_t t = 0; t < tap_list.size(); ++t) pack(&tapw[2 * t], t, tap_list[t]);
    std::copy(consts.begin(), consts.end(), scalw.begin() + consts_at);
    const struct {
        DevBuf& dev;
        const std::vector<uint32_t>& host;
        size_t least;
    } tables[3] = {{code, stream, 1}, {taps, tapw, 2}, {scal, scalw, 1}};
    for (const auto& t : tables) BX_TRY(t.dev.alloc(c, std::max(t.host.size(), t.least)));
    for (const auto& t : tables)
        if (!t.host.empty()) BX_HIP(c, hipMemcpyAsync(t.dev.b.dptr, t.host.data(), t.host.size() * 4, hipMemcpyHostToDevice, c->stream));
    BX_HIP(c, stream_wait(c));
    return nullptr;
}

// An interpreting kernel whose slot files need more dynamic LDS than a kernel may use by default asks for the largest slot files
// (set once per process and kernel; cheap to repeat).  false = the attribute could not be set.
inline bool reserve_slot_lds(const void* kernel, size_t lds) {
    return lds <= 64 * 1024 || hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BX_CONS_MAX_NARROW * 1024 + BX_CONS_MAX_WIDE * 4096) == hipSuccess;
}

// A generated kernel on a loaded program ("Generated kernels" of bx_program.h): none unless fn is set.
struct GenKernel {
    uint32_t digest[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the digest of the program this was loaded from: what a kernel must have been built from
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
};
// what tells the kinds apart in attach and detach (program_gen.cpp)
struct GenKind {
    const char* who;            // "bx_cons_program": leads every refusal, before "_attach_kernel" / "_detach_kernel"
    const char* kernel;         // the kernel's name in the code object
    const char* abi_symbol;     // the device symbols of one and of eight words
    const char* digest_symbol;
    uint32_t abi;               // the ABI number this library launches
};
// program_gen.cpp.  attach: refused by name before anything reaches HIP — a kernel already attached, an image without a code object's
// magic — and with the module unloaded again — no such kernel, a missing symbol, another ABI, another digest.  detach: drains the
// stream, then release; refused when nothing is attached.  release: unloads what is attached (no-op when nothing is; the caller has
// drained the stream).
const char* gen_attach(bx_ctx* c, GenKernel& g, const GenKind& k, const void* image, size_t len);
const char* gen_detach(bx_ctx* c, GenKernel& g, const GenKind& k);
void gen_release(GenKernel& g);

}  // namespace bx
