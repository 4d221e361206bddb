// wit_program_gen.hpp — the frame of a GENERATED witness kernel (include/bx_program.h, "Generated witness kernels", is the normative
// text).  bx_wit_program_emit_hip (cons_program_emit.cpp) writes a witness program's compiled stream as straight-line C++: one
// function template
//     template <class A> BX_WP_FN void bx_wp_body(const A& at)
// over an accessor `at` that provides the tap reads and the stores.  This header is everything around that body, once:
//   ABI       bx_wp_gen_args, the one by-value argument of the kernel, and BX_WP_ABI, its version
//   accessors WpDevAccess (device: global loads and stores, wave-uniform column offsets) and WpHostAccess (host arrays)
//   wrappers  BX_WP_WRAPPERS, which the emitted text ends with:
//               under hipcc            extern "C" __global__ bx_wp_run(bx_wp_gen_args): one lane per row, lanes with r >= n return,
//                                      no LDS, no barrier; and the two symbols bx_wit_program_attach_kernel reads back, bx_wp_abi and
//                                      bx_wp_digest (BX_WP_DIGEST_WORDS, defined by the emitted text before it includes this header)
//               under a host compiler  bx_wp_run_host(args): the body over all rows of host arrays
// A file of its own, not a part of cons_program_gen.hpp: every generated constraint text includes that header, and a code object
// is only as old as the newest file it was built from.  Nothing a constraint kernel includes changes here.
// Values are canonical throughout, by the same functions as the interpreter's opcode bodies (wit_program.hip) and the host executor
// (bx_wit_program_run_host): canonical words are unique, so the three agree word for word.  No inline assembly, nothing per lane
// indexed at run time: a slot is a local.
//
// Aliasing.  The interpreter reads and writes `data` through ONE pointer that is not __restrict__; in straight-line code that keeps
// the compiler from moving any tap load above any earlier store, and scheduling the loads early is most of what a generated kernel
// has to offer.  The device accessor therefore holds TWO views of the data group: `rdata`, const __restrict__, for taps, and
// `wdata`, __restrict__, for stores.  That is sound because no word this launch writes is read by any lane of it, which the three
// rules of the header give:
//   forwarding   a GET of a derived column at back 0 after its SET is no instruction at all: the stored var is forwarded
//   other rows   a GET of a derived column at back > 0 is refused at create
//   order        a GET of a derived column before its SET is refused at create
// so every CP_TAP of group 1 names a FREE column and every CP_ST a DERIVED one: the set of words accessed through `rdata` and the
// set accessed through `wdata` are disjoint over the whole launch, each modified word is accessed through `wdata` only, and
// `code` is another buffer (bx_wit_program_run refuses an overlap).  That is what __restrict__ promises.  The compiler takes such a
// promise from a function's PARAMETERS, not from the members of a struct, so the kernel hands the three pointers to bx_wp_lane, whose
// parameters carry it into the inlined body; a segment of a long program is a function of its own that sees the accessor by
// reference, and inside it loads stay behind earlier stores (segment tuning is out of scope).  The promise rests on the
// text having been emitted from a program that bx_wit_program_create compiled; the digest check of attach ties a code object to such
// a program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fp.hpp"

#ifndef BX_WP_ABI
#define BX_WP_ABI 1u  // the layout of bx_wp_gen_args and the meaning of its fields; a kernel built for another number is refused
#endif

struct bx_wp_gen_args {
    uint32_t* data;        // N x w_data, column-major: free columns read, derived columns written
    const uint32_t* code;  // N x w_code
    uint32_t n, po2;       // n = 1 << po2
};

#if defined(__HIPCC__)
#define BX_WP_FN __device__ __forceinline__
#define BX_WP_SEG __device__ __noinline__  // a segment of a long program: a function of its own (cons_program_emit.cpp)
#else
#define BX_WP_FN static inline
#define BX_WP_SEG static
#endif

namespace bx {

#if defined(__HIPCC__)
// one lane's view of a launch: a tap is one global load at group_base + (col << po2) + row(back), the column offset wave-uniform
struct WpDevAccess {
    const uint32_t* __restrict__ ecode;
    const uint32_t* __restrict__ rdata;  // the free columns ("Aliasing" above)
    uint32_t* __restrict__ wdata;        // the derived columns: the same buffer
    uint32_t r, n, sh;
    __device__ __forceinline__ uint32_t row(uint32_t back) const { return (r - back) & (n - 1u); }  // n divides 2^32
    __device__ __forceinline__ uint32_t code(uint32_t col, uint32_t rb) const { return ecode[((size_t)col << sh) + rb]; }
    __device__ __forceinline__ uint32_t data(uint32_t col, uint32_t rb) const { return rdata[((size_t)col << sh) + rb]; }
    __device__ __forceinline__ void store(uint32_t col, uint32_t v) const { wdata[((size_t)col << sh) + r] = v; }
};
#else
struct WpHostAccess {
    const uint32_t* ecode;
    uint32_t* edata;
    uint32_t r, n, sh;
    uint32_t row(uint32_t back) const { return (r - back) & (n - 1u); }
    uint32_t code(uint32_t col, uint32_t rb) const { return ecode[((size_t)col << sh) + rb]; }
    uint32_t data(uint32_t col, uint32_t rb) const { return edata[((size_t)col << sh) + rb]; }
    void store(uint32_t col, uint32_t v) const { edata[((size_t)col << sh) + r] = v; }
};
#endif

}  // namespace bx

#if defined(__HIPCC__)
#define BX_WP_WRAPPERS                                                                                                          \
    extern "C" __device__ __attribute__((used)) const uint32_t bx_wp_digest[8] = {BX_WP_DIGEST_WORDS};                          \
    extern "C" __device__ __attribute__((used)) const uint32_t bx_wp_abi = BX_WP_ABI;                                           \
    static __device__ __forceinline__ void bx_wp_lane(const uint32_t* __restrict__ code, const uint32_t* __restrict__ rdata,    \
                                                      uint32_t* __restrict__ wdata, uint32_t r, uint32_t n, uint32_t po2) {     \
        const bx::WpDevAccess at{code, rdata, wdata, r, n, po2};                                                                \
        bx_wp_body(at);                                                                                                         \
    }                                                                                                                           \
    extern "C" __global__ __launch_bounds__(256) void bx_wp_run(bx_wp_gen_args a) {                                            \
        const uint32_t r = blockIdx.x * 256u + threadIdx.x;                                                                     \
        if (r >= a.n) return;                                                                                                   \
        bx_wp_lane(a.code, a.data, a.data, r, a.n, a.po2);                                                                      \
    }
#else
#define BX_WP_WRAPPERS                                                                                                          \
    static const uint32_t bx_wp_digest[8] = {BX_WP_DIGEST_WORDS};                                                               \
    static const uint32_t bx_wp_abi = BX_WP_ABI;                                                                                \
    static inline void bx_wp_run_host(const bx_wp_gen_args& a) {                                                                \
        for (uint32_t r = 0; r < a.n; ++r) {                                                                                    \
            const bx::WpHostAccess at{a.code, a.data, r, a.n, a.po2};                                                           \
            bx_wp_body(at);                                                                                                     \
        }                                                                                                                       \
    }
#endif
