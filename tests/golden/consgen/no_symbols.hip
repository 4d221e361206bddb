// A refusal fixture of tests/test_consgen_gpu.py: a valid gfx950 code object with none of the three symbols a generated
// constraint-program kernel carries (bx_cp_eval, bx_cp_abi, bx_cp_digest).  bx_cons_program_attach_kernel must refuse it by name.
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" __global__ void trivial_fill(uint32_t* out, uint32_t n, uint32_t v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v;
}
