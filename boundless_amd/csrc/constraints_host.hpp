// constraints_host.hpp — what the verifier-side `constraints_at` of the built-in circuits share (circuit_host.cpp, lookup_host.cpp):
// reading tap values through the verifier's bx_tap_reader, and the running sum_i poly_mix^i C_i.  Host arithmetic only.
#pragma once
#include "../../include/bx_circuit.h"
#include "fp.hpp"

namespace bx {

// Tap values by (group, column, rows back).  A tap the verifier refuses reads as zero and its error sticks: the circuit evaluates
// on and hands `err` back with its result.
struct TapValues {
    const bx_tap_reader* taps;
    const char* err = nullptr;
    Fp4 at(int g, uint32_t c, int back) {
        Fp4 v = f4_zero();
        if (const char* e = taps->at(taps->ctx, g, c, back, v.c)) err = e;
        return v;
    }
    // the ext-valued column s of the accum group: sum_k X^k * column(4s+k)
    Fp4 ext_at(uint32_t s, int back) {
        Fp4 r = f4_zero();
        for (int k = 0; k < 4; ++k) {
            Fp4 xk = f4_zero();
            xk.c[k] = MONT_ONE;
            r = f4_add(r, f4_mul(xk, at(2, 4 * s + k, back)));
        }
        return r;
    }
};

// sum_i poly_mix^i C_i, one constraint at a time in the circuit's order
struct MixedSum {
    Fp4 poly_mix, rhs = f4_zero(), cur = f4_one();
    void add(const Fp4& cons) {
        rhs = f4_add(rhs, f4_mul(cur, cons));
        cur = f4_mul(cur, poly_mix);
    }
};

}  // namespace bx
