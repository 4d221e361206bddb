// circuit_host.cpp — verifier side of the synthetic circuit (include/bx_prover.h): sum_i poly_mix^i C_i from the tap values, the
// polynomial eval_check_kernel (circuit.hip) evaluates over the 4N domain.  Host arithmetic only.
#include <string.h>

#include "circuit.hpp"
#include "constraints_host.hpp"

namespace bx {
const char* synthetic_constraints_at(void*, const bx_segment_params* shape, const bx_tap_reader* taps, const uint32_t poly_mix_w[4],
                                     const uint32_t mix_w[4], const uint32_t* globals, uint32_t out[4]) {
    const Circuit cc = circuit_of(shape);
    const Fp4 beta{{mix_w[0], mix_w[1], mix_w[2], mix_w[3]}};
    TapValues tv{taps};
    MixedSum sum{Fp4{{poly_mix_w[0], poly_mix_w[1], poly_mix_w[2], poly_mix_w[3]}}};
    for (uint32_t j = 0; j < cc.J; ++j) {
        Fp4 pool[Circuit::POOL];
        for (unsigned slot = 0; slot < Circuit::POOL; ++slot) {
            const Circuit::Src src = cc.pool_src(j, slot);
            pool[slot] = src.group < 0 ? f4_one() : tv.at(src.group, src.col, src.back);
        }
        Fp4 cell = f4_zero();
        for (uint32_t t = 0; t < cc.T; ++t) {
            Fp4 prod = pool[Circuit::pool_idx(t, 0)];
            for (uint32_t f = 1; f < cc.G; ++f) prod = f4_mul(prod, pool[Circuit::pool_idx(t, f)]);
            cell = f4_add(cell, prod);
        }
        sum.add(f4_sub(tv.at(1, cc.F + j, 0), cell));
    }
    const Fp4 first = tv.at(0, 0, 0);
    Fp4 be = beta;
    for (uint32_t e = 0; e < cc.E; ++e) {
        const Fp4 inner = f4_add(first, f4_mul(f4_sub(f4_one(), first), tv.ext_at(e, 1)));
        sum.add(f4_sub(tv.ext_at(e, 0), f4_mul(inner, f4_add(be, tv.at(1, cc.acc_src(e), 0)))));
        if (e & 1) be = f4_mul(be, beta);  // beta^(floor(e/2)+1)
    }
    for (uint32_t p = 0; p < cc.pairs; ++p) sum.add(f4_mul(tv.at(0, 1, 0), f4_sub(tv.ext_at(2 * p + 1, 0), tv.ext_at(2 * p, 0))));
    // boundary constraints tying the public words to the trace
    sum.add(f4_mul(first, f4_sub(tv.at(1, 0, 0), Fp4{{globals[0], 0u, 0u, 0u}})));
    if (cc.globals() > 1) sum.add(f4_mul(tv.at(0, 1, 0), f4_sub(tv.at(1, cc.wd - 1, 0), Fp4{{globals[1], 0u, 0u, 0u}})));
    memcpy(out, sum.rhs.c, 16);
    return tv.err;
}
}  // namespace bx
