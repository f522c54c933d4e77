// kmath_ops.h -- one op of kmath.h applied to one item of raw words: what
// khp_kmath_host (kmath_host.cpp, the host compiler) and khp_debug_kmath (flatten.hip,
// gfx950) both run, so that a test can hold each compile of kmath.h to a truth and the
// two to one another.  The item layout is kirk_hip.h's (khp_kmath_op): three 64-bit words
// in, three out, nothing converted on the way.
#pragma once

#include "../../include/kirk_hip.h"
#include "kmath.h"

namespace khp {

constexpr uint32_t KMATH_MAX_ITEMS = 1u << 20;
constexpr int KMATH_WORDS = 3;   // per item, in and out

KHD float km_lo(uint64_t w) { return f_from_bits((uint32_t)w); }
KHD float km_hi(uint64_t w) { return f_from_bits((uint32_t)(w >> 32)); }
KHD uint64_t km_f(float f) { return (uint64_t)bits_from_f(f); }
KHD void km_st3(uint64_t* o, v3 a) {
    o[0] = km_f(a.x);
    o[1] = km_f(a.y);
    o[2] = km_f(a.z);
}

// the 64 x 64 -> high 64 product as env_light.h's env_scale_u24 takes it
KHD uint64_t km_umulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// op is in [0, KHP_KMATH_OP_COUNT): the callers check it.
KHD void kmath_apply(uint32_t op, const uint64_t* w, uint64_t* o) {
    const float a = km_lo(w[0]), b = km_lo(w[1]), c = km_lo(w[2]);
    const uint32_t ua = (uint32_t)w[0], ub = (uint32_t)w[1], uc = (uint32_t)w[2];
    const double da = d_from_bits(w[0]), db = d_from_bits(w[1]);
    const v3 p = mk(km_lo(w[0]), km_hi(w[0]), km_lo(w[1])), q = mk(km_hi(w[1]), km_lo(w[2]), km_hi(w[2]));
    o[0] = o[1] = o[2] = 0;
    switch (op) {
    case KHP_KMATH_MUL: o[0] = km_f(a * b); break;
    case KHP_KMATH_ADD: o[0] = km_f(a + b); break;
    case KHP_KMATH_DIV: o[0] = km_f(a / b); break;
    case KHP_KMATH_SQRT: o[0] = km_f(sqrtf(a)); break;
    case KHP_KMATH_RSQRT: o[0] = km_f(1.0f / sqrtf(a)); break;
    case KHP_KMATH_MULADD: {
        float t = a * b;
        t = t + c;
        o[0] = km_f(t);
        break;
    }
    case KHP_KMATH_FLOOR: o[0] = km_f(floorf(a)); break;
    case KHP_KMATH_F2I: o[0] = (uint64_t)(uint32_t)(int)a; break;
    case KHP_KMATH_F2U: o[0] = (uint64_t)(uint32_t)a; break;
    case KHP_KMATH_I2F: o[0] = km_f((float)(int)ua); break;
    case KHP_KMATH_U2F: o[0] = km_f((float)ua); break;
    case KHP_KMATH_U642F: o[0] = km_f((float)w[0]); break;
    case KHP_KMATH_D2I2D: o[0] = bits_from_d((double)(int64_t)da); break;
    case KHP_KMATH_DMUL: o[0] = bits_from_d(da * db); break;
    case KHP_KMATH_DADD: o[0] = bits_from_d(da + db); break;
    case KHP_KMATH_DDIV: o[0] = bits_from_d(da / db); break;
    case KHP_KMATH_UMULHI: o[0] = km_umulhi(w[0], w[1]); break;
    case KHP_KMATH_LDEXPF: o[0] = km_f(k_ldexpf(a, (int)ub)); break;
    case KHP_KMATH_SINF: o[0] = km_f(k_sinf(a)); break;
    case KHP_KMATH_COSF: o[0] = km_f(k_cosf(a)); break;
    case KHP_KMATH_ATANF: o[0] = km_f(k_atanf(a)); break;
    case KHP_KMATH_ATAN2F: o[0] = km_f(k_atan2f(a, b)); break;
    case KHP_KMATH_ASINF: o[0] = km_f(k_asinf(a)); break;
    case KHP_KMATH_ACOSF: o[0] = km_f(k_acosf(a)); break;
    case KHP_KMATH_EXPF: o[0] = km_f(k_expf(a)); break;
    case KHP_KMATH_SINHF: o[0] = km_f(k_sinhf(a)); break;
    case KHP_KMATH_HYPOTF: o[0] = km_f(k_hypotf(a, b)); break;
    case KHP_KMATH_LOGF_D: o[0] = km_f(k_logf_d(a)); break;
    case KHP_KMATH_POWF_D: o[0] = km_f(k_powf_d(a, b)); break;
    case KHP_KMATH_J0: o[0] = bits_from_d(k_j0(da)); break;
    case KHP_KMATH_LOG_D: o[0] = bits_from_d(k_log_d(da)); break;
    case KHP_KMATH_EXP_D: o[0] = bits_from_d(k_exp_d(da)); break;
    case KHP_KMATH_POW_D: o[0] = bits_from_d(k_pow_d(da, db)); break;
    case KHP_KMATH_LOWBIAS32: o[0] = (uint64_t)lowbias32(ua); break;
    case KHP_KMATH_PATH_KEY: o[0] = (uint64_t)path_key(ua, ub, uc); break;
    case KHP_KMATH_DRAW_U32: o[0] = (uint64_t)draw_u32(ua, ub); break;
    case KHP_KMATH_DRAW_U01: o[0] = km_f(draw_u01(ua, ub)); break;
    case KHP_KMATH_DOT: o[0] = km_f(dot(p, q)); break;
    case KHP_KMATH_CROSS: km_st3(o, cross(p, q)); break;
    case KHP_KMATH_NORMALIZE: km_st3(o, normalize(p)); break;
    case KHP_KMATH_REFLECT: km_st3(o, reflect(p, q)); break;
    case KHP_KMATH_REFRACT: km_st3(o, refract(p, q, q.z)); break;
    case KHP_KMATH_ROTATE_ROWVEC: km_st3(o, rotate_rowvec(p, q.x, mk(q.y, q.z, p.z))); break;
    case KHP_KMATH_ANGLE: o[0] = km_f(angle(p, q)); break;
    case KHP_KMATH_FACEFORWARD: km_st3(o, faceforward(p, q, p)); break;
    case KHP_KMATH_GMIN: o[0] = km_f(gmin(a, b)); break;
    case KHP_KMATH_GMAX: o[0] = km_f(gmax(a, b)); break;
    case KHP_KMATH_GCLAMP: o[0] = km_f(gclamp(a, b, c)); break;
    default: break;
    }
}

// The checks the two entries share; null: the call is fine.
inline const char* kmath_args_error(uint32_t op, uint32_t n, const void* in, const void* out) {
    if (!in || !out) return "null argument";
    if (op >= (uint32_t)KHP_KMATH_OP_COUNT) return "unknown op";
    if (n == 0u || n > KMATH_MAX_ITEMS) return "n must be in [1, 2^20]";
    return nullptr;
}

}  // namespace khp
