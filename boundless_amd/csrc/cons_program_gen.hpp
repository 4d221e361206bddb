// cons_program_gen.hpp — the frame of a GENERATED eval_check (include/bx_program.h, "Generated kernels", is the normative text).
// bx_cons_program_emit_hip (cons_program_emit.cpp) writes a program's compiled stream as straight-line C++: one function template
//     template <class A> BX_CP_FN bx::Fp4 bx_cp_body(const A& at)
// over an accessor `at` that provides the tap, scalar and mix-power reads.  This header is everything around that body, once:
//   ABI       bx_cp_gen_args, the one by-value argument of the kernel, and BX_CP_ABI, its version
//   accessors CpDevAccess (device: global loads, wave-uniform column offsets and table reads) and CpHostAccess (host arrays)
//   closing   cp_store_check: the division by zinv[i & 3] into the four check planes, as store_check of circuit_common.hpp
//   wrappers  BX_CP_WRAPPERS, which the emitted text ends with:
//               under hipcc            extern "C" __global__ bx_cp_eval(bx_cp_gen_args): one lane per domain point, lanes past `dom`
//                                      return, no LDS; and the two symbols bx_cons_program_attach_kernel reads back, bx_cp_abi and
//                                      bx_cp_digest (BX_CP_DIGEST_WORDS, defined by the emitted text before it includes this header)
//               under a host compiler  bx_cp_eval_host(args): the four planes over the whole domain from host arrays, and
//                                      bx_cp_body_at(args, i): the body's value at one point (tests/test_consgen_cpu.py)
// Values are canonical throughout, by the same functions as the interpreter's opcode bodies (cons_program.hip): canonical words are
// unique, so the two executors agree word for word.  No inline assembly, nothing per lane indexed at run time: a slot is a local.
#pragma once
#ifndef BX_PLAIN_MAD
#define BX_PLAIN_MAD 1  // the multiply-adds of lazy_ext.hpp as plain C++, on the device too
#endif
#include <stddef.h>
#include <stdint.h>

#include "fp.hpp"
#include "lazy_ext.hpp"

#ifndef BX_CP_ABI
#define BX_CP_ABI 1u  // the layout of bx_cp_gen_args and the meaning of its fields; a kernel built for another number is refused
#endif

struct bx_cp_gen_args {
    uint32_t* check;        // 4 planes of `dom` words
    const uint32_t* ecode;  // the three evaluation groups, dom x width column-major
    const uint32_t* edata;
    const uint32_t* eacc;
    const uint32_t* scal;     // [globals | mix (4)]: what changes per call (the program's constants are literals of the text)
    const uint32_t* mixpows;  // canonical powers of poly_mix, four words each
    uint32_t zinv[4];         // 1 / (3^N w_4^m - 1), m = row mod 4
    uint32_t dom, po2;        // dom = 4 << po2
};

#if defined(__HIPCC__)
#define BX_CP_FN __device__ __forceinline__
#define BX_CP_SEG __device__ __noinline__  // a segment of a long program: a function of its own (cons_program_emit.cpp)
#else
#define BX_CP_FN static inline
#define BX_CP_SEG static
#endif

namespace bx {

BX_HD Fp4 cp_add_eb(Fp4 x, uint32_t y) {
    x.c[0] = fp_add(x.c[0], y);
    return x;
}
BX_HD Fp4 cp_sub_eb(Fp4 x, uint32_t y) {
    x.c[0] = fp_sub(x.c[0], y);
    return x;
}
BX_HD Fp4 cp_sub_be(uint32_t x, const Fp4& y) { return Fp4{{fp_sub(x, y.c[0]), fp_neg(y.c[1]), fp_neg(y.c[2]), fp_neg(y.c[3])}}; }

#if defined(__HIPCC__)
// one lane's view of a launch: a tap is one global load at group_base + (col << (po2 + 2)) + row(back), the column offset wave-uniform
struct CpDevAccess {
    const uint32_t* __restrict__ ecode;
    const uint32_t* __restrict__ edata;
    const uint32_t* __restrict__ eacc;
    const uint32_t* __restrict__ scal;
    const uint32_t* __restrict__ mixpows;
    uint32_t i, dom, sh;
    __device__ __forceinline__ uint32_t row(uint32_t back) const { return (i - 4u * back) & (dom - 1u); }  // dom divides 2^32
    __device__ __forceinline__ uint32_t code(uint32_t col, uint32_t r) const { return ecode[((size_t)col << sh) + r]; }
    __device__ __forceinline__ uint32_t data(uint32_t col, uint32_t r) const { return edata[((size_t)col << sh) + r]; }
    __device__ __forceinline__ uint32_t accum(uint32_t col, uint32_t r) const { return eacc[((size_t)col << sh) + r]; }
    __device__ __forceinline__ uint32_t scalar(uint32_t k) const { return scal[k]; }
    __device__ __forceinline__ Fp4 power(uint32_t k) const {
        const uint4 m = *reinterpret_cast<const uint4*>(mixpows + 4 * (size_t)k);
        return Fp4{{m.x, m.y, m.z, m.w}};
    }
};
__device__ __forceinline__ void cp_store_check(uint32_t* __restrict__ check, const Fp4& tot, const uint32_t (&zinv)[4], uint32_t dom, uint32_t i) {
    const Fp4 q = f4_scale(tot, zinv[i & 3u]);
#pragma unroll
    for (int k = 0; k < 4; ++k) check[(size_t)k * dom + i] = q.c[k];
}
#else
struct CpHostAccess {
    const uint32_t* ecode;
    const uint32_t* edata;
    const uint32_t* eacc;
    const uint32_t* scal;
    const uint32_t* mixpows;
    uint32_t i, dom, sh;
    uint32_t row(uint32_t back) const { return (i - 4u * back) & (dom - 1u); }
    uint32_t code(uint32_t col, uint32_t r) const { return ecode[((size_t)col << sh) + r]; }
    uint32_t data(uint32_t col, uint32_t r) const { return edata[((size_t)col << sh) + r]; }
    uint32_t accum(uint32_t col, uint32_t r) const { return eacc[((size_t)col << sh) + r]; }
    uint32_t scalar(uint32_t k) const { return scal[k]; }
    Fp4 power(uint32_t k) const { return Fp4{{mixpows[4 * (size_t)k], mixpows[4 * (size_t)k + 1], mixpows[4 * (size_t)k + 2], mixpows[4 * (size_t)k + 3]}}; }
};
#endif

}  // namespace bx

#if defined(__HIPCC__)
#define BX_CP_WRAPPERS                                                                                                          \
    extern "C" __device__ __attribute__((used)) const uint32_t bx_cp_digest[8] = {BX_CP_DIGEST_WORDS};                          \
    extern "C" __device__ __attribute__((used)) const uint32_t bx_cp_abi = BX_CP_ABI;                                           \
    extern "C" __global__ __launch_bounds__(256) void bx_cp_eval(bx_cp_gen_args a) {                                           \
        const uint32_t i = blockIdx.x * 256u + threadIdx.x;                                                                     \
        if (i >= a.dom) return;                                                                                                 \
        const bx::CpDevAccess at{a.ecode, a.edata, a.eacc, a.scal, a.mixpows, i, a.dom, a.po2 + 2u};                            \
        bx::cp_store_check(a.check, bx_cp_body(at), a.zinv, a.dom, i);                                                          \
    }
#else
#define BX_CP_WRAPPERS                                                                                                          \
    static const uint32_t bx_cp_digest[8] = {BX_CP_DIGEST_WORDS};                                                               \
    static const uint32_t bx_cp_abi = BX_CP_ABI;                                                                                \
    static inline bx::Fp4 bx_cp_body_at(const bx_cp_gen_args& a, uint32_t i) {                                                  \
        const bx::CpHostAccess at{a.ecode, a.edata, a.eacc, a.scal, a.mixpows, i, a.dom, a.po2 + 2u};                           \
        return bx_cp_body(at);                                                                                                  \
    }                                                                                                                           \
    static inline void bx_cp_eval_host(const bx_cp_gen_args& a) {                                                               \
        for (uint32_t i = 0; i < a.dom; ++i) {                                                                                  \
            const bx::Fp4 q = bx::f4_scale(bx_cp_body_at(a, i), a.zinv[i & 3u]);                                                \
            for (int k = 0; k < 4; ++k) a.check[(size_t)k * a.dom + i] = q.c[k];                                                \
        }                                                                                                                       \
    }
#endif
