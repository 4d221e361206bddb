// cons_program_exec.hpp — one instruction of a compiled program for one lane: the opcode bodies the interpreting kernels share
// (cons_program.hip over the 4N domain, acc_program.hip and wit_program.hip over the N trace rows).  Device only; the including
// translation unit defines BX_PLAIN_MAD first (circuit_common.hpp).  What differs between the kernels comes through `Env`:
//   EXT          does the kind have ext values (CP_LD_E, CP_ADD_EB .. CP_MUL_EE); when not, their bodies are not compiled and `wid`
//                is never touched
//   MIX          does the stream hold the mix opcodes (CP_ZERO .. CP_COND_E); when not, their bodies are not compiled
//   tap(imm)     the word tap imm reads for this lane
//   mixpows()    the canonical mix-power table (MIX only)
//   other(...)   any opcode this file does not know (CP_ST of a witness program, the term stores of an accumulate program; nothing
//                for a constraint program)
// The slot files live in LDS, slot-major: narrow slot s of lane t is nar[256 s], wide slot s four such planes (cons_program.hip).
// No index is checked here: a stream reaches a kernel only through a load, which holds it against program_fits (cons_program.hpp).
#pragma once
#include "circuit_common.hpp"
#include "cons_program.hpp"

namespace bx {

constexpr uint32_t CP_LANES = 256;

__device__ __forceinline__ Fp4 cp_ldw(const uint32_t* wid, uint32_t s) {
    const uint32_t* p = wid + 4 * s * CP_LANES;
    return Fp4{{p[0], p[CP_LANES], p[2 * CP_LANES], p[3 * CP_LANES]}};
}
__device__ __forceinline__ void cp_stw(uint32_t* wid, uint32_t s, const Fp4& v) {
    uint32_t* p = wid + 4 * s * CP_LANES;
    p[0] = v.c[0];
    p[CP_LANES] = v.c[1];
    p[2 * CP_LANES] = v.c[2];
    p[3 * CP_LANES] = v.c[3];
}

// everything decoded from w0 / w1 is wave-uniform
template <class Env>
__device__ __forceinline__ void cp_exec(uint32_t w0v, uint32_t w1v, uint32_t* nar, uint32_t* wid, const uint32_t* __restrict__ scal, const Env& env) {
    const uint32_t w0 = __builtin_amdgcn_readfirstlane(w0v), w1 = __builtin_amdgcn_readfirstlane(w1v);
    const uint32_t op = w0 & 0xFFu, dst = (w0 >> 8) & 0xFFu, a = (w0 >> 16) & 0xFFu, b = w0 >> 24, c = w1 & 0xFFu, imm = w1 >> 8;
    switch (op) {
    case CP_NOP: break;
    case CP_LD_B: nar[dst * CP_LANES] = scal[imm]; break;
    case CP_LD_E:
        if constexpr (Env::EXT) {
            const uint32_t* s = scal + imm;
            cp_stw(wid, dst, Fp4{{s[0], s[1], s[2], s[3]}});
        }
        break;
    case CP_TAP: nar[dst * CP_LANES] = env.tap(imm); break;
    case CP_ADD_BB: nar[dst * CP_LANES] = fp_add(nar[a * CP_LANES], nar[b * CP_LANES]); break;
    case CP_SUB_BB: nar[dst * CP_LANES] = fp_sub(nar[a * CP_LANES], nar[b * CP_LANES]); break;
    case CP_MUL_BB: nar[dst * CP_LANES] = fp_mul(nar[a * CP_LANES], nar[b * CP_LANES]); break;
    case CP_ADD_EB:
        if constexpr (Env::EXT) {
            Fp4 x = cp_ldw(wid, a);
            x.c[0] = fp_add(x.c[0], nar[b * CP_LANES]);
            cp_stw(wid, dst, x);
        }
        break;
    case CP_SUB_EB:
        if constexpr (Env::EXT) {
            Fp4 x = cp_ldw(wid, a);
            x.c[0] = fp_sub(x.c[0], nar[b * CP_LANES]);
            cp_stw(wid, dst, x);
        }
        break;
    case CP_SUB_BE:
        if constexpr (Env::EXT) {
            const Fp4 y = cp_ldw(wid, b);
            cp_stw(wid, dst, Fp4{{fp_sub(nar[a * CP_LANES], y.c[0]), fp_neg(y.c[1]), fp_neg(y.c[2]), fp_neg(y.c[3])}});
        }
        break;
    case CP_MUL_EB:
        if constexpr (Env::EXT) cp_stw(wid, dst, f4_scale(cp_ldw(wid, a), nar[b * CP_LANES]));
        break;
    case CP_ADD_EE:
        if constexpr (Env::EXT) cp_stw(wid, dst, f4_add(cp_ldw(wid, a), cp_ldw(wid, b)));
        break;
    case CP_SUB_EE:
        if constexpr (Env::EXT) cp_stw(wid, dst, f4_sub(cp_ldw(wid, a), cp_ldw(wid, b)));
        break;
    case CP_MUL_EE:
        if constexpr (Env::EXT) cp_stw(wid, dst, f4_mul_lz(cp_ldw(wid, a), cp_ldw(wid, b)));
        break;
    case CP_ZERO:
        if constexpr (Env::MIX) cp_stw(wid, dst, f4_zero());
        break;
    case CP_EQZ_B:
        if constexpr (Env::MIX) cp_stw(wid, dst, f4_add(cp_ldw(wid, a), f4_scale(mix_power(env.mixpows(), imm), nar[b * CP_LANES])));
        break;
    case CP_EQZ_E:
        if constexpr (Env::MIX) cp_stw(wid, dst, f4_add(cp_ldw(wid, a), f4_mul_lz(mix_power(env.mixpows(), imm), cp_ldw(wid, b))));
        break;
    case CP_COND_B:
        if constexpr (Env::MIX) {
            const Fp4 w = f4_mul_lz(mix_power(env.mixpows(), imm), cp_ldw(wid, c));
            cp_stw(wid, dst, f4_add(cp_ldw(wid, a), f4_scale(w, nar[b * CP_LANES])));
        }
        break;
    case CP_COND_E:
        if constexpr (Env::MIX) {
            const Fp4 w = f4_mul_lz(mix_power(env.mixpows(), imm), cp_ldw(wid, c));
            cp_stw(wid, dst, f4_add(cp_ldw(wid, a), f4_mul_lz(w, cp_ldw(wid, b))));
        }
        break;
    default: env.other(op, a, b, imm, nar, wid); break;
    }
}

}  // namespace bx
