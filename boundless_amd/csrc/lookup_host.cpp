// lookup_host.cpp — verifier side of the lookup circuit (include/bx_lookup.h): sum_i poly_mix^i C_i from the tap values, the
// polynomial lookup_eval_check_kernel (lookup.hip) evaluates over the 4N domain.  Host arithmetic only.
#include <string.h>

#include "constraints_host.hpp"
#include "lookup.hpp"

namespace bx {
const char* lookup_constraints_at(void*, const bx_segment_params* shape, const bx_tap_reader* taps, const uint32_t poly_mix_w[4], const uint32_t mix_w[4],
                                  const uint32_t* globals, uint32_t out[4]) {
    const Lookup lk = lookup_of(shape);
    const Fp4 alpha{{mix_w[0], mix_w[1], mix_w[2], mix_w[3]}};
    TapValues tv{taps};
    MixedSum sum{Fp4{{poly_mix_w[0], poly_mix_w[1], poly_mix_w[2], poly_mix_w[3]}}};
    const uint32_t mont_b = fp_encode(lk.B);
    for (uint32_t j = 0; j < lk.V; ++j)
        sum.add(f4_sub(f4_sub(tv.at(1, 3 * j, 0), tv.at(1, 3 * j + 1, 0)), f4_scale(tv.at(1, 3 * j + 2, 0), mont_b)));
    const Fp4 first = tv.at(0, 0, 0), last = tv.at(0, 1, 0), not_first = f4_sub(f4_one(), first);
    Fp4 total = f4_zero();
    for (uint32_t s = 0; s <= 2 * lk.V; ++s) {
        const Fp4 cur_sum = tv.ext_at(s, 0);
        const Fp4 step = f4_sub(cur_sum, f4_mul(not_first, tv.ext_at(s, 1)));
        total = f4_add(total, cur_sum);
        if (s < 2 * lk.V) sum.add(f4_sub(f4_mul(step, f4_sub(alpha, tv.at(1, lk.limb_col(s), 0))), f4_one()));
        else sum.add(f4_add(f4_mul(step, f4_sub(alpha, tv.at(0, 2, 0))), tv.at(1, lk.mult_col(), 0)));
    }
    sum.add(f4_mul(last, total));
    const Fp4 v0 = tv.at(1, 0, 0);
    sum.add(f4_mul(first, f4_sub(v0, Fp4{{globals[0], 0u, 0u, 0u}})));
    sum.add(f4_mul(last, f4_sub(v0, Fp4{{globals[1], 0u, 0u, 0u}})));
    memcpy(out, sum.rhs.c, 16);
    return tv.err;
}
}  // namespace bx
