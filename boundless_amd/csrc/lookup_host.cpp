// lookup_host.cpp — verifier side of the lookup circuit (include/bx_lookup.h): sum_i poly_mix^i C_i from the tap values, the
// polynomial lookup_eval_check_kernel (lookup.hip) evaluates over the 4N domain.  Host arithmetic only.
#include <string.h>

#include "fp.hpp"
#include "lookup.hpp"

namespace bx {
const char* lookup_constraints_at(void*, const bx_segment_params* shape, const bx_tap_reader* taps, const uint32_t poly_mix_w[4], const uint32_t mix_w[4],
                                  const uint32_t* globals, uint32_t out[4]) {
    const Lookup lk = lookup_of(shape);
    const Fp4 poly_mix{{poly_mix_w[0], poly_mix_w[1], poly_mix_w[2], poly_mix_w[3]}}, alpha{{mix_w[0], mix_w[1], mix_w[2], mix_w[3]}};
    const char* err = nullptr;
    auto at = [&](int g, uint32_t c, int back) -> Fp4 {
        Fp4 v = f4_zero();
        if (const char* e = taps->at(taps->ctx, g, c, back, v.c)) err = e;
        return v;
    };
    auto sum_at = [&](uint32_t s, int back) -> Fp4 {  // the ext-valued running sum: sum_k X^k * column(4s+k)
        Fp4 r = f4_zero();
        for (int k = 0; k < 4; ++k) {
            Fp4 xk = f4_zero();
            xk.c[k] = MONT_ONE;
            r = f4_add(r, f4_mul(xk, at(2, 4 * s + k, back)));
        }
        return r;
    };
    Fp4 rhs = f4_zero(), cur = f4_one();
    auto mix_in = [&](const Fp4& cons) {
        rhs = f4_add(rhs, f4_mul(cur, cons));
        cur = f4_mul(cur, poly_mix);
    };
    const uint32_t mont_b = fp_encode(lk.B);
    for (uint32_t j = 0; j < lk.V; ++j)
        mix_in(f4_sub(f4_sub(at(1, 3 * j, 0), at(1, 3 * j + 1, 0)), f4_scale(at(1, 3 * j + 2, 0), mont_b)));
    const Fp4 first = at(0, 0, 0), last = at(0, 1, 0), not_first = f4_sub(f4_one(), first);
    Fp4 total = f4_zero();
    for (uint32_t s = 0; s <= 2 * lk.V; ++s) {
        const Fp4 cur_sum = sum_at(s, 0);
        const Fp4 step = f4_sub(cur_sum, f4_mul(not_first, sum_at(s, 1)));
        total = f4_add(total, cur_sum);
        if (s < 2 * lk.V) mix_in(f4_sub(f4_mul(step, f4_sub(alpha, at(1, lk.limb_col(s), 0))), f4_one()));
        else mix_in(f4_add(f4_mul(step, f4_sub(alpha, at(0, 2, 0))), at(1, lk.mult_col(), 0)));
    }
    mix_in(f4_mul(last, total));
    const Fp4 v0 = at(1, 0, 0);
    mix_in(f4_mul(first, f4_sub(v0, Fp4{{globals[0], 0u, 0u, 0u}})));
    mix_in(f4_mul(last, f4_sub(v0, Fp4{{globals[1], 0u, 0u, 0u}})));
    memcpy(out, rhs.c, 16);
    return err;
}
}  // namespace bx
