// hair_lobes.h -- MarschnerHairBSDF::localSample with its TT and TRT fibre paths
// (Common/Shading/Bsdf.cpp:491-663, 737-766), the three-call state machine KIRK
// carries across bounces in Bounce::mat_flags and switches off with `int p = 0;`
// (:669).  Included by device.h after hair_r; bsdf_sample's Marschner case calls
// hair_lobes() in the kernel instances compiled with KINDS_LOBES (khp_set_hair_lobes
// with a lobe other than R), and hair_r -- the p = 0 answer -- in all the others.
//
//   unflagged          first hit: p = hair_lobe_pick(lobes, u).  p = 0 is hair_r;
//                      p = 1 / 2 refract into the fibre with 1/ior, flags = CYL_T /
//                      CYL_TR, f = 0
//   CYL_T, not CYL_TR  TT exit (:492-568), flags = 0
//   CYL_TR, not CYL_T  reflection at the far wall (:573-580), flags |= CYL_T |
//                      SPECULAR, f = 0
//   CYL_TR and CYL_T   TRT exit (:581-662), flags = 0
//
// Kept as written in the reference: the diffuse colour is the absorption sigma;
// TT's cos_gamma_t is -2 cos(asin(h / eta')); TRT carries a factor 10; both exits
// refract with eta = 1 (the ray leaves unbent) and the lobe shift alpha, drawn in
// degrees, goes to glm::rotate as radians.  float32 throughout, except TRT's
// dh_dphi, which the reference computes in double (std::_Pi, :642).
#pragma once

namespace khp {

constexpr uint32_t HAIR_LOBE_R = 1u, HAIR_LOBE_TT = 2u, HAIR_LOBE_TRT = 4u, HAIR_LOBE_ALL = 7u;

// The lobe of a first hit: the k-th enabled one in the order R, TT, TRT with
// k = min(count - 1, (int)(u * count)); KIRK's uniform_int_distribution(0, 2)
// (:667) is the all-three case.  One enabled lobe needs no draw.
KHD int hair_lobe_pick(uint32_t lobes, float u) {
    const int count = (int)(lobes & 1u) + (int)((lobes >> 1) & 1u) + (int)((lobes >> 2) & 1u);
    int k = (int)(u * (float)count);
    k = k < count - 1 ? k : count - 1;
    for (int p = 0; p < 3; ++p)
        if ((lobes >> p) & 1u) {
            if (k == 0) return p;
            --k;
        }
    return 0;
}

// The exits' shared terms: gamma_i, the Bravais indices and dialectricFresnel (:528-553, :618-645)
struct HairAzimuth {
    float gi, h, b1, b2, c, F;
};
__device__ __forceinline__ HairAzimuth hair_azimuth(v3 nin, v3 n, float ior) {
    HairAzimuth a;
    a.gi = angle(nin, normalize(n));
    float cgi = k_cosf(a.gi);
    float sgi = k_sinf(a.gi);
    float x1 = sqrtf(ior * ior - sgi * sgi);
    a.b1 = x1 / cgi;
    a.b2 = ior * ior * cgi / x1;
    a.c = k_asinf(1.0f / a.b1);
    a.h = k_sinf(a.gi);
    a.F = fresnel_dielectric(a.gi, a.b1, a.b2);
    return a;
}

__device__ __forceinline__ v3 hair_lobes(const ShadeCtx& s, v3 in, v3 n, float sample[2], float h0, float h1,
                                         float lobe_u, uint32_t lobes, v3& out, float& pdf, int& flags) {
    const v3 zero = mk(0.0f, 0.0f, 0.0f);
    const bool t = (flags & F_CYL_T) != 0, tr = (flags & F_CYL_TR) != 0;
    float ior = s.m->ior;
    v3 nin = normalize(in);
    if (!t && !tr) {  // :664-767
        const int p = hair_lobe_pick(lobes, lobe_u);
        if (p == 0) return hair_r<false>(s, in, n, sample, h0, h1, out, pdf, flags);
        out = refract(-nin, faceforward(n, -nin, n), 1.0f / ior);
        flags = p == 1 ? F_CYL_T : F_CYL_TR;
        return zero;
    }
    if (tr && !t) {  // :573-580
        out = reflect(-nin, faceforward(n, -nin, n));
        flags |= F_CYL_T | F_SPECULAR;
        return zero;
    }
    v3 in_cyl = world_to_local(in, s.V, s.U, s.W);
    float alpha = -1.0f * (5.0f + 5.0f * h0);
    float beta = 5.0f + 5.0f * h1;
    v3 diff = mk(s.m->diffuse[0], s.m->diffuse[1], s.m->diffuse[2]);
    v3 o1 = refract(-nin, faceforward(n, -nin, n), 1.0f);
    // TT shifts by -alpha/2 and narrows to beta/2 (:498, :515-519); TRT by -3 alpha/2 and 2 beta (:587, :605-609)
    const float shift = tr ? -3.0f * alpha / 2.0f : -alpha / 2.0f;
    const float sd = tr ? 2.0f * beta : beta / 2.0f;
    o1 = rotate_rowvec(o1, shift, s.V);
    flags = 0;
    v3 oc = world_to_local(o1, s.V, s.U, s.W);
    float ti = k_atan2f(k_hypotf(in_cyl.x, in_cyl.z), in_cyl.y);
    float tr_ = k_atan2f(k_hypotf(oc.x, oc.z), oc.y);
    float th = (tr_ + ti) / 2.0f;
    float td = (tr_ - ti) / 2.0f;
    float gx = th - shift;
    out = o1;
    sample[0] = ti;
    sample[1] = 0.0f;
    pdf = normal_gauss_pdf(gx, 0.0f, sd);
    const HairAzimuth a = hair_azimuth(nin, n, ior);
    v3 sigma = diff / k_cosf(tr_);
    float ctd = k_cosf(td);
    if (!tr) {  // TT exit, :541-567
        float dh = 1.0f / fabsf((1.0f / sqrtf(1.0f - a.h * a.h)) *
                                ((-(24.0f * a.c / (PIF * PIF * PIF)) * (a.gi * a.gi)) + (6.0f * a.c / PIF - 2.0f)));
        float cgt = -2.0f * k_cosf(k_asinf(a.h / a.b1));
        float w = (1.0f - a.F) * (1.0f - a.F);
        v3 e = sigma * cgt;
        v3 att = mk(k_expf(e.x), k_expf(e.y), k_expf(e.z)) * w;
        v3 ntt = (att * 0.5f) * dh;
        return (ntt * pdf) / (ctd * ctd);
    }
    // TRT exit, :620-661
    const double pi3 = M_PI_D * M_PI_D * M_PI_D;
    float dh = (float)(1.0 / fabs((double)(1.0f / sqrtf(1.0f - a.h * a.h)) *
                                  (-((double)(48.0f * a.c) / pi3) * (double)(a.gi * a.gi) +
                                   ((double)(12.0f * a.c) / M_PI_D - 2.0))));
    float gt = k_asinf(a.h / a.b1);
    float cgt = k_cosf(gt);
    float Fx = fresnel_dielectric(gt, 1.0f / a.b1, 1.0f / a.b2);
    float w = ((1.0f - a.F) * (1.0f - a.F)) * Fx;
    v3 e = sigma * (-2.0f * cgt);
    v3 ex = mk(k_expf(e.x), k_expf(e.y), k_expf(e.z));
    v3 att = (ex * ex) * w;
    v3 ntrt = (att * 0.5f) * dh;
    return ((ntrt * pdf) / (ctd * ctd)) * 10.0f;
}

}  // namespace khp
