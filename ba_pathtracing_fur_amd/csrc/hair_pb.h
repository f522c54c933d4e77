// hair_pb.h -- BSDF kind 11, KHP_BSDF_CHIANG_HAIR: the near-field fibre model of Chiang,
// Bitterli, Tappan and Burley (2016) with its four lobes R, TT, TRT and the residual,
// importance sampled and evaluated with its true value.  It is not KIRK's:
// KIRK's two hair BSDFs stay as written (device.h: hair_r, hair_lobes.h).
// Plain float32 functions compiled by g++ (hair_pb_host.cpp: khp_hair_eval_host,
// khp_hair_sample_host) and by hipcc (device.h: bsdf_sample / bsdf_eval of the instances
// whose KINDS holds bit 11), both with -ffp-contract=off: the same bits on host and device.
// Every step is one float32 operation in the order written.
#pragma once

#include <stdint.h>

#include "../../include/kirk_hip.h"
#include "kmath.h"

namespace khp {

constexpr float HAIR_2PI = 6.28318530717958647692f;      // 2 pi rounded to float32
constexpr float HAIR_LN2 = 0.693147180559945309417f;     // ln 2 rounded to float32
constexpr float HAIR_SQRT_PI_8 = 0.626657069f;           // sqrt(pi / 8): the logistic scale of beta_n

// Why khp_hair_material, khp_set_scene and khp_host_build refuse material m of kind 11, or null.
inline const char* hair_material_error(const khp_material& m) {
    auto in01 = [](float b) { return b >= 0.01f && b <= 1.0f; };
    if (m.shader != KHP_SHADER_SIMPLE) return "a ChiangHairBSDF material takes KHP_SHADER_SIMPLE";
    if (!in01(m.roughness)) return "ChiangHairBSDF: beta_m (roughness) must be in [0.01, 1]";
    if (!in01(m.specular[0])) return "ChiangHairBSDF: beta_n (specular[0]) must be in [0.01, 1]";
    if (!(m.specular[1] >= -30.0f && m.specular[1] <= 30.0f)) return "ChiangHairBSDF: alpha (specular[1]) must be in [-30, 30] degrees";
    if (m.specular[2] != 0.0f) return "ChiangHairBSDF: specular[2] is reserved and must be 0";
    if (!(m.ior > 1.0f) || m.ior == k_inf()) return "ChiangHairBSDF: ior must be finite and > 1";
    for (int c = 0; c < 3; ++c)
        if (!(m.volume[c] >= 0.0f) || m.volume[c] == k_inf()) return "ChiangHairBSDF: sigma_a (volume) must be finite and >= 0";
    return nullptr;
}

// Dielectric Fresnel reflectance (KIRK's BSDF::fresnelDielectric, Bsdf.cpp:143-171): the
// function every BSDF of device.h calls, here so the host entries compile it too.
KHD float fresnel_dielectric(float cos_theta, float eta_i, float eta_t) {
    float ci = gclamp(cos_theta, -1.0f, 1.0f);
    if (ci <= 0.0f) {
        float t = eta_i;
        eta_i = eta_t;
        eta_t = t;
        ci = fabsf(ci);
    }
    float si = sqrtf(gmax(0.0f, 1.0f - ci * ci));
    float st = eta_i / eta_t * si;
    if (st >= 1.0f) return 1.0f;
    float ct = sqrtf(gmax(0.0f, 1.0f - st * st));
    float rparl = ((eta_t * ci) - (eta_i * ct)) / ((eta_t * ci) + (eta_i * ct));
    float rperp = ((eta_i * ci) - (eta_t * ct)) / ((eta_i * ci) + (eta_t * ct));
    return (rparl * rparl + rperp * rperp) / 2.0f;
}

KHD float hp_ssqrt(float x) { return sqrtf(gmax(x, 0.0f)); }
KHD float hp_sasin(float x) { return k_asinf(gclamp(x, -1.0f, 1.0f)); }

// I0s: the first ten terms of the power series of the modified Bessel function I0.
KHD float hp_i0s(float x) {
    const float x2 = x * x;
    float val = 0.0f, x2i = 1.0f, ifact = 1.0f, i4 = 1.0f;
    for (int i = 0; i < 10; ++i) {
        if (i > 1) ifact = ifact * (float)i;
        val = val + x2i / (i4 * (ifact * ifact));
        x2i = x2i * x2;
        i4 = i4 * 4.0f;
    }
    return val;
}
KHD float hp_log_i0(float x) {
    if (x <= 8.0f) return k_logf_d(hp_i0s(x));
    return ((x - 0.5f * k_logf_d(HAIR_2PI * x)) + 1.0f / (8.0f * x)) + 1.0f / (16.0f * (x * x));
}
KHD float hp_i0(float x) {
    if (x <= 8.0f) return hp_i0s(x);
    return k_expf(hp_log_i0(x));
}

// The longitudinal lobe M_p.
KHD float hp_mp(float cti, float cto, float sti, float sto, float v) {
    const float a = (cti * cto) / v, b = (sti * sto) / v;
    if (v <= 0.1f) return k_expf((((hp_log_i0(a) - b) - 1.0f / v) + HAIR_LN2) + k_logf_d(1.0f / (2.0f * v)));
    return (k_expf(-b) * hp_i0(a)) / (k_sinhf(1.0f / v) * (2.0f * v));
}
KHD float hp_logistic(float x, float s) {
    const float e = k_expf(-(fabsf(x) / s));
    return e / (s * ((1.0f + e) * (1.0f + e)));
}
KHD float hp_logistic_cdf(float x, float s) { return 1.0f / (1.0f + k_expf(-(x / s))); }
KHD float hp_phi(int p, float gamma_o, float gamma_t) {
    return ((2.0f * (float)p) * gamma_t - 2.0f * gamma_o) + (float)p * PIF;
}
// The azimuthal lobe N_p: the logistic of scale s about Phi(p), trimmed to [-pi, pi].
KHD float hp_np(float phi, int p, float s, float gamma_o, float gamma_t) {
    float d = phi - hp_phi(p, gamma_o, gamma_t);
    for (int k = 0; k < 4 && d > PIF; ++k) d = d - HAIR_2PI;   // |d| < 8 pi: `while`, bounded
    for (int k = 0; k < 4 && d < -PIF; ++k) d = d + HAIR_2PI;
    return hp_logistic(d, s) / (hp_logistic_cdf(PIF, s) - hp_logistic_cdf(-PIF, s));
}

// What one hit fixes: the outgoing direction in the fibre's frame, the lobe widths, the
// cuticle tilt and the attenuations A_p.
struct HairHit {
    float sto, cto, phio;       // w_o: sin and cos of theta_o, phi_o
    float gamma_o, gamma_t;
    float v[4], s;
    float s2k[3], c2k[3];
    v3 A[4];
};

KHD float hp_pow20(float x, float& x22) {
    const float x2 = x * x, x4 = x2 * x2, x8 = x4 * x4, x16 = x8 * x8, x20 = x16 * x4;
    x22 = x20 * x2;
    return x20;
}

// U, V, W, n: surface_at's frame and normal; wo: the unit direction to the viewer.
KHD void hair_hit(const khp_material& m, v3 U, v3 V, v3 W, v3 n, v3 wo, HairHit& H) {
    const float eta = m.ior;
    const float bm = gclamp(m.roughness, 0.01f, 1.0f), bn = gclamp(m.specular[0], 0.01f, 1.0f);
    H.sto = dot(wo, V);
    H.cto = hp_ssqrt(1.0f - H.sto * H.sto);
    H.phio = k_atan2f(dot(wo, W), dot(wo, U));
    const v3 np = dot(wo, n) >= 0.0f ? n : -n;
    const float phin = k_atan2f(dot(np, W), dot(np, U));
    float go = H.phio - phin;
    for (int k = 0; k < 4 && go > PIF; ++k) go = go - HAIR_2PI;   // |go| <= 2 pi: `while`, bounded
    for (int k = 0; k < 4 && go < -PIF; ++k) go = go + HAIR_2PI;
    const float h = gclamp(k_sinf(go), -1.0f, 1.0f);
    H.gamma_o = hp_sasin(h);
    float unused;
    const float b20 = hp_pow20(bm, unused);
    float b22;
    hp_pow20(bn, b22);
    const float l = (0.726f * bm + 0.812f * (bm * bm)) + 3.7f * b20;
    const float v0 = l * l;
    H.v[0] = v0;
    H.v[1] = 0.25f * v0;
    H.v[2] = 4.0f * v0;
    H.v[3] = 4.0f * v0;
    H.s = HAIR_SQRT_PI_8 * ((0.265f * bn + 1.194f * (bn * bn)) + 5.372f * b22);
    H.s2k[0] = k_sinf(m.specular[1] * DEG2RAD);
    H.c2k[0] = hp_ssqrt(1.0f - H.s2k[0] * H.s2k[0]);
    for (int i = 1; i < 3; ++i) {
        H.s2k[i] = (2.0f * H.c2k[i - 1]) * H.s2k[i - 1];
        H.c2k[i] = H.c2k[i - 1] * H.c2k[i - 1] - H.s2k[i - 1] * H.s2k[i - 1];
    }
    const float stt = H.sto / eta;
    const float ctt = hp_ssqrt(1.0f - stt * stt);
    const float etap = sqrtf(eta * eta - H.sto * H.sto) / H.cto;
    const float sgt = h / etap;
    const float cgt = hp_ssqrt(1.0f - sgt * sgt);
    H.gamma_t = hp_sasin(sgt);
    const float len = (2.0f * cgt) / ctt;
    const v3 T = mk(k_expf(-(m.volume[0] * len)), k_expf(-(m.volume[1] * len)), k_expf(-(m.volume[2] * len)));
    const float F = fresnel_dielectric(H.cto * hp_ssqrt(1.0f - h * h), 1.0f, eta);
    const float omf = 1.0f - F;
    H.A[0] = mk(F, F, F);
    H.A[1] = T * (omf * omf);
    H.A[2] = (H.A[1] * T) * F;
    const v3 num = (H.A[2] * F) * T;
    const v3 den = mk(1.0f - T.x * F, 1.0f - T.y * F, 1.0f - T.z * F);
    H.A[3] = mk(den.x > 0.0f ? num.x / den.x : 0.0f, den.y > 0.0f ? num.y / den.y : 0.0f,
                den.z > 0.0f ? num.z / den.z : 0.0f);
}

// The outgoing angles of lobe p, tilted by the cuticle; p = 3 is untilted.
KHD void hp_tilt(const HairHit& H, int p, float& stp, float& ctp) {
    if (p == 0) {
        stp = H.sto * H.c2k[1] - H.cto * H.s2k[1];
        ctp = H.cto * H.c2k[1] + H.sto * H.s2k[1];
    } else if (p == 1) {
        stp = H.sto * H.c2k[0] + H.cto * H.s2k[0];
        ctp = H.cto * H.c2k[0] - H.sto * H.s2k[0];
    } else if (p == 2) {
        stp = H.sto * H.c2k[2] + H.cto * H.s2k[2];
        ctp = H.cto * H.c2k[2] - H.sto * H.s2k[2];
    } else {
        stp = H.sto;
        ctp = H.cto;
    }
    ctp = fabsf(ctp);
}

// The lobe terms of S(w_o, w_i) that do not depend on the weights: M_p N_p for p < 3 and
// M_3 / (2 pi) enter S as (M_p a_p) N_p and (M_3 a_3) / (2 pi).
struct HairLobes {
    float m[4];   // M_p
    float n[3];   // N_p(phi_i - phi_o)
};
KHD void hp_lobes(const HairHit& H, v3 U, v3 V, v3 W, v3 wi, HairLobes& L) {
    const float sti = dot(wi, V);
    const float cti = hp_ssqrt(1.0f - sti * sti);
    const float phi = k_atan2f(dot(wi, W), dot(wi, U)) - H.phio;
    for (int p = 0; p < 4; ++p) {
        float stp, ctp;
        hp_tilt(H, p, stp, ctp);
        L.m[p] = hp_mp(cti, ctp, sti, stp, H.v[p]);
    }
    for (int p = 0; p < 3; ++p) L.n[p] = hp_np(phi, p, H.s, H.gamma_o, H.gamma_t);
}
// S with the weights a_p in place of A_p (one channel).
KHD float hp_sum(const HairLobes& L, float a0, float a1, float a2, float a3) {
    const float t0 = (L.m[0] * a0) * L.n[0];
    const float t1 = (L.m[1] * a1) * L.n[1];
    const float t2 = (L.m[2] * a2) * L.n[2];
    const float t3 = (L.m[3] * a3) / HAIR_2PI;
    return ((t0 + t1) + t2) + t3;
}
// f = S / |dot(w_i, n)| (S itself where the dot is 0): both shader sites multiply by it.
KHD v3 hp_value(const HairHit& H, const HairLobes& L, v3 n, v3 wi) {
    v3 S = mk(hp_sum(L, H.A[0].x, H.A[1].x, H.A[2].x, H.A[3].x), hp_sum(L, H.A[0].y, H.A[1].y, H.A[2].y, H.A[3].y),
              hp_sum(L, H.A[0].z, H.A[1].z, H.A[2].z, H.A[3].z));
    const float c = fabsf(dot(wi, n));
    if (c != 0.0f) S = S / c;
    return S;
}

// f(w_o, w_i): wo to the viewer, wi to the light, any length (normalised here).
KHD v3 hair_pb_eval(const khp_material& m, v3 U, v3 V, v3 W, v3 n, v3 wo, v3 wi) {
    if (is_zero(V)) return mk(0.0f, 0.0f, 0.0f);
    wo = normalize(wo);
    wi = normalize(wi);
    HairHit H;
    hair_hit(m, U, V, W, n, wo, H);
    HairLobes L;
    hp_lobes(H, U, V, W, wi, L);
    return hp_value(H, L, n, wi);
}

// One sample of w_i given w_o and the four draws u_l, u_n, u_0, u_1; returns f(w_o, out).
KHD v3 hair_pb_sample(const khp_material& m, v3 U, v3 V, v3 W, v3 n, v3 wo, float ul, float un, float u0, float u1,
                      v3& out, float& pdf, bool& valid) {
    const v3 zero = mk(0.0f, 0.0f, 0.0f);
    out = mk(0.0f, 0.0f, 1.0f);
    pdf = 0.0f;
    valid = false;
    if (is_zero(V)) return zero;
    wo = normalize(wo);
    HairHit H;
    hair_hit(m, U, V, W, n, wo, H);
    float w[4];
    for (int p = 0; p < 4; ++p) w[p] = (H.A[p].x + H.A[p].y) + H.A[p].z;
    const float tot = ((w[0] + w[1]) + w[2]) + w[3];
    if (!(tot > 0.0f)) return zero;
    float q[4];
    for (int p = 0; p < 4; ++p) q[p] = w[p] / tot;
    int p = 3;
    float run = q[0];
    if (ul < run) p = 0;
    else {
        run = run + q[1];
        if (ul < run) p = 1;
        else {
            run = run + q[2];
            if (ul < run) p = 2;
        }
    }
    float stp, ctp;
    hp_tilt(H, p, stp, ctp);
    u0 = gmax(u0, 1e-5f);
    const float vp = H.v[p];
    const float ct = 1.0f + vp * k_logf_d(u0 + (1.0f - u0) * k_expf(-2.0f / vp));
    const float st = hp_ssqrt(1.0f - ct * ct);
    const float sti = -ct * stp + (st * k_cosf(HAIR_2PI * u1)) * ctp;
    const float cti = hp_ssqrt(1.0f - sti * sti);
    float dphi;
    if (p < 3) {
        const float cm = hp_logistic_cdf(-PIF, H.s), cp = hp_logistic_cdf(PIF, H.s);
        const float x = -H.s * k_logf_d(1.0f / (un * (cp - cm) + cm) - 1.0f);
        dphi = hp_phi(p, H.gamma_o, H.gamma_t) + gclamp(x, -PIF, PIF);
    } else {
        dphi = HAIR_2PI * un;
    }
    const float phii = H.phio + dphi;
    out = (V * sti + U * (cti * k_cosf(phii))) + W * (cti * k_sinf(phii));
    // S is a function of the two directions: f and pdf both take their angles from `out`,
    // as hair_pb_eval(wo, out) does, so that call returns this f bit for bit.
    const v3 wi = normalize(out);
    HairLobes L;
    hp_lobes(H, U, V, W, wi, L);
    pdf = hp_sum(L, q[0], q[1], q[2], q[3]);
    valid = true;
    return hp_value(H, L, n, wi);
}

}  // namespace khp
