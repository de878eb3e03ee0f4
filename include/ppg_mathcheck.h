/*
 * ppg_mathcheck.h — ONE definition of "evaluate function `op` of the shared numerical contract (ppg_detmath.h, ppg_rng.h) on this input",
 * shared by everything that checks the contract: the oracle (ppgo_math_eval, ppgo_math_checksum: g++), the HIP library's host code
 * (ppg_debug_math_* with family = -1: clang's host pass, the compiler behind csrc/ppg_scene_build.h) and the debug kernels of every kernel
 * family (csrc/ppg_debug_kernels.h: the gfx950 back end).  The contract is that all three give the same bits for every input of an op's
 * DOMAIN: the inputs for which every C++ step of the function is defined.  Inputs outside it are never evaluated by a checker.
 *
 * Arguments and results travel as bit patterns (uint32_t), so that NaN payloads and integer words pass through unchanged.
 *
 *   op  function                                   a               b               o0           o1
 *    0  ppg_sincos(a)                              float           -               sin          cos
 *    1  ppg_atan2(a, b)                            float y         float x         float        -
 *    2  ppg_exp(a)                                 float           -               float        -
 *    3  ppg_from_fixed(ppg_to_fixed(a))            float           -               float        -
 *    4  ppg_rand(key, (uint32_t)b)                 key, as bits    float dim       float        -     (ppgo_math_eval and ppg_debug_math_eval
 *                                                                                                      derive the key from the element's index:
 *                                                                                                      ppg_mathcheck_arg_a)
 *    5  ppg_powi(a, (int)b)                        float           float n         float        -
 *    6  ppg_log(a)                                 float           -               float        -
 *    7  ppg_pow(a, b)                              float x         float y         float        -
 *    8  ppg_rand(ppg_path_key(seed, pixel, sample), dim)   pixel   seed << 16 | sample << 4 | dim     float   -
 *    9  ppg_adam_learning_rate(0.01, 0.9, 0.999, (int)a)   float iter   -          float        -
 *   10  ppg_atan(a)                                float           -               float        -
 *   11  ppg_acos(a)                                float           -               float        -
 *   12  ppg_tan(a)                                 float           -               float        -
 *   13  ppg_to_fixed(a), raw                       float           -               low word     high word
 *   14  ppg_to_sfixed(a), raw                      float           -               low word     high word
 *   15  ppg_from_fixed(b << 32 | a)                low word        high word       float        -
 *   16  ppg_from_sfixed((int64_t)(b << 32 | a))    low word        high word       float        -
 */
#ifndef PPG_MATHCHECK_H
#define PPG_MATHCHECK_H

#include "ppg_detmath.h"
#include "ppg_rng.h"

#define PPG_MATHCHECK_OPS 17
#define PPG_MATHCHECK_BLOCK_BITS 24 /* the 2^32 float patterns are 256 blocks of 2^24: pattern = block << 24 | index */
#define PPG_MATHCHECK_BLOCKS 256

PPG_HD bool ppg_mathcheck_known(int op) { return op >= 0 && op < PPG_MATHCHECK_OPS; }
/* the ops of ONE argument: those a block checksum over the float patterns exists for */
PPG_HD bool ppg_mathcheck_unary(int op) { return op == 0 || op == 2 || op == 3 || op == 6 || (op >= 9 && op <= 14); }
/* how many of (o0, o1) the op writes, and how many of them are floats (a NaN among those is canonicalised by the checksum) */
PPG_HD int ppg_mathcheck_outputs(int op) { return (op == 0 || op == 13 || op == 14) ? 2 : 1; }
PPG_HD int ppg_mathcheck_float_outputs(int op) { return op == 0 ? 2 : ((op == 13 || op == 14) ? 0 : 1); }
/* the ops the kernels call through an out-of-line copy of their module (csrc/ppg_device.h): dm_sincos, dm_atan2, dm_exp, dm_log, dm_pow,
   dm_acos, dm_tan */
PPG_HD bool ppg_mathcheck_has_dm(int op) { return op == 0 || op == 1 || op == 2 || op == 6 || op == 7 || op == 11 || op == 12; }

/* "Every C++ step of `op` is defined for (a, b)".  What limits a domain is a float-to-integer conversion, undefined in C++ (and different
   between x86-64 and gfx950 in practice) where the truncated value does not fit the integer type:
     sincos, tan          |x| <= 2^30 (the quadrant index (int)(|x| 4/pi) fits; NaN is outside)
     adam_learning_rate   1 <= iter <= 2^24
     powi                 0 <= n < 4096
     ppg_rand, op 4       -1 < dim < 2^32
   Every other op takes every input, NaN, the infinities and the denormals included — ppg_log of a denormal and ppg_exp beyond +-80 are
   useless values (ppg_detmath.h), but defined arithmetic must agree all the same.  ppg_exp (and with it ppg_pow) converts a NaN to int on
   its way; whatever that gives, the result is NaN times a power of two: NaN on every side, which is all the checks look at. */
PPG_HD bool ppg_mathcheck_in_domain(int op, uint32_t a, uint32_t b) {
    const float fa = ppg_u2f(a), fb = ppg_u2f(b);
    switch (op) {
        case 0: case 12: return ppg_abs(fa) <= 1073741824.0f;
        case 4: return fb > -1.0f && fb < 4294967296.0f;
        case 5: return fb >= 0.0f && fb < 4096.0f;
        case 9: return fa >= 1.0f && fa <= 16777216.0f;
        default: return ppg_mathcheck_known(op);
    }
}

/* The one evaluator.  Callers check ppg_mathcheck_known and ppg_mathcheck_in_domain first; *o1 is written only by ops of two outputs. */
PPG_HD void ppg_mathcheck_eval(int op, uint32_t a, uint32_t b, uint32_t *o0, uint32_t *o1) {
    const float fa = ppg_u2f(a), fb = ppg_u2f(b);
    switch (op) {
        case 0: { float s, c; ppg_sincos(fa, &s, &c); *o0 = ppg_f2u(s); *o1 = ppg_f2u(c); break; }
        case 1: *o0 = ppg_f2u(ppg_atan2(fa, fb)); break;
        case 2: *o0 = ppg_f2u(ppg_exp(fa)); break;
        case 3: *o0 = ppg_f2u(ppg_from_fixed(ppg_to_fixed(fa))); break;
        case 4: *o0 = ppg_f2u(ppg_rand(a, (uint32_t)fb)); break;
        case 5: *o0 = ppg_f2u(ppg_powi(fa, (int)fb)); break;
        case 6: *o0 = ppg_f2u(ppg_log(fa)); break;
        case 7: *o0 = ppg_f2u(ppg_pow(fa, fb)); break;
        case 8: *o0 = ppg_f2u(ppg_rand(ppg_path_key((uint64_t)(b >> 16), a, (b >> 4) & 0xfffu), b & 15u)); break;
        case 9: *o0 = ppg_f2u(ppg_adam_learning_rate(0.01f, 0.9f, 0.999f, (int)fa)); break;
        case 10: *o0 = ppg_f2u(ppg_atan(fa)); break;
        case 11: *o0 = ppg_f2u(ppg_acos(fa)); break;
        case 12: *o0 = ppg_f2u(ppg_tan(fa)); break;
        case 13: { const uint64_t r = ppg_to_fixed(fa); *o0 = (uint32_t)r; *o1 = (uint32_t)(r >> 32); break; }
        case 14: { const uint64_t r = (uint64_t)ppg_to_sfixed(fa); *o0 = (uint32_t)r; *o1 = (uint32_t)(r >> 32); break; }
        case 15: *o0 = ppg_f2u(ppg_from_fixed(((uint64_t)b << 32) | a)); break;
        case 16: *o0 = ppg_f2u(ppg_from_sfixed((int64_t)(((uint64_t)b << 32) | a))); break;
        default: break;
    }
}

/* Element i of an element-wise evaluation: op 4 draws from the key of the element's index, every other op from a[i] as it stands. */
PPG_HD uint32_t ppg_mathcheck_arg_a(int op, uint32_t i, uint32_t a) { return op == 4 ? i * 2654435761u + 17u : a; }

/* The checksum of a block is the wrapping 64-bit sum, over the block's inputs u inside the domain (b = 0), of this term: a fixed
   multiply-xorshift of (u, o0, o1), NaN results canonicalised first because their payloads may legitimately differ.  A sum: the order
   in which lanes, waves and threads add their terms does not matter. */
PPG_HD uint32_t ppg_mathcheck_canon(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u : bits; }
PPG_HD uint64_t ppg_mathcheck_mix(uint32_t u, uint32_t o0, uint32_t o1) {
    uint64_t h = ((uint64_t)u + 1u) * 0x9e3779b97f4a7c15ull;
    h ^= ((uint64_t)o1 << 32) | o0;
    h ^= h >> 32; h *= 0xd6e8feb86659fd93ull;
    h ^= h >> 32; h *= 0xd6e8feb86659fd93ull;
    h ^= h >> 32;
    return h;
}
PPG_HD uint64_t ppg_mathcheck_term(int op, uint32_t u) {
    if (!ppg_mathcheck_in_domain(op, u, 0u)) return 0ull;
    uint32_t o0 = 0u, o1 = 0u;
    ppg_mathcheck_eval(op, u, 0u, &o0, &o1);
    const int nf = ppg_mathcheck_float_outputs(op);
    if (nf > 0) o0 = ppg_mathcheck_canon(o0);
    if (nf > 1) o1 = ppg_mathcheck_canon(o1);
    return ppg_mathcheck_mix(u, o0, o1);
}

#endif /* PPG_MATHCHECK_H */
