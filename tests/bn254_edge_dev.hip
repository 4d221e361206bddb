// bn254_edge_dev.hip — the gfx950 build of the BN254 edge-operand op table (tests/bn254_edge_ops.hpp): one lane per record, one
// kernel per op family, and a small runner on the C ABI that tests/bn254_edge.py loads with ctypes.
//
// One file, six translation units (hipcc's time on the curve kernels is minutes, so tests/bn254_edge.py compiles them in parallel):
// with -DBN_EDGE_FAMILY=<n> it is family n's kernel and its launch function; without, it is the runner that calls the five.
#include <hip/hip_runtime.h>

#include "bn254_edge_ops.hpp"

using namespace bn_edge;

#define BN_EDGE_CAT2(a, b) a##b
#define BN_EDGE_CAT(a, b) BN_EDGE_CAT2(a, b)

#ifdef BN_EDGE_FAMILY

namespace {

template <uint32_t FAMILY>
__global__ __launch_bounds__(64) void edge_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    constexpr uint32_t NIN = FAMILY <= FIELD_R ? FIELD_IN : FAMILY == FQ2 ? FQ2_IN : FAMILY == CURVE_Q ? CurveWords<Fq>::IN : CurveWords<Fq2>::IN;
    constexpr uint32_t NOUT = FAMILY <= FIELD_R ? FIELD_OUT : FAMILY == FQ2 ? FQ2_OUT : FAMILY == CURVE_Q ? CurveWords<Fq>::OUT : CurveWords<Fq2>::OUT;
    const uint32_t* rec = in + (size_t)i * NIN;
    uint32_t* res = out + (size_t)i * NOUT;
    if (FAMILY == FIELD_Q) apply_field<FqP>(rec, res);
    else if (FAMILY == FIELD_R) apply_field<FrP>(rec, res);
    else if (FAMILY == FQ2) apply_fq2(rec, res);
    else if (FAMILY == CURVE_Q) apply_curve<Fq>(rec, res);
    else apply_curve<Fq2>(rec, res);
}

}  // namespace

static_assert(BN_EDGE_FAMILY < N_FAMILIES, "unknown family");
// din: count records of words_in(family) words; dout: count rows of words_out(family) words (device)
extern "C" int BN_EDGE_CAT(bn254_edge_launch_, BN_EDGE_FAMILY)(const uint32_t* din, uint32_t* dout, uint32_t count) {
    hipLaunchKernelGGL(edge_kernel<BN_EDGE_FAMILY>, dim3((count + 63) / 64), dim3(64), 0, 0, din, dout, count);
    return (int)hipGetLastError();
}

#else

extern "C" {
int bn254_edge_launch_0(const uint32_t*, uint32_t*, uint32_t);
int bn254_edge_launch_1(const uint32_t*, uint32_t*, uint32_t);
int bn254_edge_launch_2(const uint32_t*, uint32_t*, uint32_t);
int bn254_edge_launch_3(const uint32_t*, uint32_t*, uint32_t);
int bn254_edge_launch_4(const uint32_t*, uint32_t*, uint32_t);
}

// in: count records of words_in(family) words (host); out: count rows of words_out(family) words (host).  Returns the HIP error
// code (0 = ok), -1 for an unknown family or a count out of range.
extern "C" __attribute__((visibility("default"))) int bn254_edge_run(uint32_t family, const uint32_t* in, uint32_t count, uint32_t* out) {
    static int (*const launch[N_FAMILIES])(const uint32_t*, uint32_t*, uint32_t) = {bn254_edge_launch_0, bn254_edge_launch_1, bn254_edge_launch_2,
                                                                                   bn254_edge_launch_3, bn254_edge_launch_4};
    if (family >= N_FAMILIES || count == 0 || count > (1u << 24)) return -1;
    const size_t bin = (size_t)count * words_in(family) * 4, bout = (size_t)count * words_out(family) * 4;
    uint32_t *din = nullptr, *dout = nullptr;
    int e = (int)hipMalloc(&din, bin);
    if (e == 0) e = (int)hipMalloc(&dout, bout);
    if (e == 0) e = (int)hipMemcpy(din, in, bin, hipMemcpyHostToDevice);
    if (e == 0) e = (int)hipMemset(dout, 0xA5, bout);
    if (e == 0) e = launch[family](din, dout, count);
    if (e == 0) e = (int)hipDeviceSynchronize();
    if (e == 0) e = (int)hipMemcpy(out, dout, bout, hipMemcpyDeviceToHost);
    (void)hipFree(din);
    (void)hipFree(dout);
    return e;
}

#endif
