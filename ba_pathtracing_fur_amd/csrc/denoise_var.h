// denoise_var.h -- the definition of khp_denoise_var / khp_denoise_var_host (kirk_hip.h,
// DESIGN.md §17): denoise.h's guided a-trous filter with its colour distance measured in
// units of each pixel's measured noise, the variance of the pixel's mean, which is
// filtered along with the colour and can be returned.
//
// As in denoise.h everything that computes a value is a KHD function of this header,
// compiled into the host entry (denoise_var_host.cpp, g++) and into the gfx950 kernels
// (denoise_var_dev.h, included by render.hip); every operation is one float32 operation in
// the order written, nothing is contracted, and tests/_denoisevarref.py restates the same
// sequence in numpy.  What §13 defines (the guides' prepare, clamp, fin, the tap order, h,
// the non-colour terms, w, which taps count, the new colour) is taken from denoise.h's
// functions or restated here operation for operation; denoise.h itself is left as it is.
//
// Stages:
//   dnv_prepare  per pixel, denoise.h's records (n.xyz, d) (t.xyz, cv) (c.rgb, fin) and the
//                8-byte variance record (v, known);
//   dnv_filter   one iteration for one pixel: the trimmed 3 x 3 prefilter of the variance,
//                then the 25 taps, dy outer, dx inner, for the colour and the variance;
//   finish       the colour as it is, out_variance = known ? v : +inf.
// The argument checks of both entries are dnv_check.
#pragma once

#include "denoise.h"
#include "moments.h"

namespace khp {

// The variance record: the variance of the pixel's mean and whether it is known (1.0f / 0.0f).
// Every load or store of one is a single aligned 64-bit access.
struct alignas(8) DnVar {
    float v, known;
};

// The noise source as the stages use it.  mom: the context's moments state, two MomRec per pixel.
struct DnvNoise {
    uint32_t source;      // KHP_NOISE_*
    uint32_t prefilter;   // 0 or 1
    float floor;
    const float* variance;
    const float* m2;
    const uint32_t* count;
    const MomRec* mom;
    const MomRec* mean;   // not NULL: the colour is the moments' mean, read in place from the (mean, n) records
    float* out_variance;
};

// The variance of the mean of n samples whose squared deviations sum to s per channel, channels
// summed: the expression under mom_rel_error's square root, restated (moments.h stays as it is).
KHD float dnv_var_of_mean(float m2r, float m2g, float m2b, uint32_t n) {
    const float s = (m2r + m2g) + m2b;
    const float nf = (float)n;
    return s / (nf * (nf - 1.0f));
}

KHD DnVar dnv_prepare_noise(const DnvNoise& Z, size_t p) {
    float u = 0.0f;
    bool has = true;
    if (Z.source == KHP_NOISE_PLANE) {
        u = Z.variance[p];
    } else {
        float r, g, b;
        uint32_t n;
        if (Z.source == KHP_NOISE_CONTEXT) {
            const MomRec a = Z.mom[2 * p], m = Z.mom[2 * p + 1];
            r = m.x; g = m.y; b = m.z;
            n = a.w;
        } else {
            r = Z.m2[3 * p]; g = Z.m2[3 * p + 1]; b = Z.m2[3 * p + 2];
            n = Z.count[p];
        }
        has = n >= 2u;
        if (has) u = dnv_var_of_mean(r, g, b, n);
    }
    const bool known = has && dn_finite(u) && u >= 0.0f;
    DnVar v;
    v.v = known ? u : 0.0f;
    v.known = known ? 1.0f : 0.0f;
    return v;
}

// §13's prepare without demodulation; the colour is the caller's plane or the moments' mean.
KHD void dnv_prepare(const DnParams& P, const DnPlanes& G, const DnvNoise& Z, size_t p, DnRec& g0, DnRec& g1, DnRec& col,
                     DnVar& var) {
    const float cv = dn_reads_coverage(P.on) ? G.coverage[p] : 0.0f;
    const float inv = cv > 0.0f ? 1.0f / cv : 0.0f;
    g0.x = g0.y = g0.z = g0.w = 0.0f;
    g1.x = g1.y = g1.z = 0.0f;
    g1.w = cv;
    if (P.on & DN_NORMAL) dn_unit(G.normal + 3 * p, inv, g0.x, g0.y, g0.z);
    if (P.on & DN_TANGENT) dn_unit(G.tangent + 3 * p, inv, g1.x, g1.y, g1.z);
    if (P.on & DN_DEPTH) g0.w = G.depth[p] * inv;
    float c[3];
    if (Z.mean) {
        const MomRec a = Z.mean[2 * p];
        c[0] = a.x; c[1] = a.y; c[2] = a.z;
    } else {
        c[0] = G.colour[3 * p]; c[1] = G.colour[3 * p + 1]; c[2] = G.colour[3 * p + 2];
    }
    if (P.clamp > 0.0f)
        for (int k = 0; k < 3; ++k) c[k] = c[k] > P.clamp ? P.clamp : c[k];   // NaN and -inf pass
    col.x = c[0];
    col.y = c[1];
    col.z = c[2];
    col.w = (dn_finite(c[0]) && dn_finite(c[1]) && dn_finite(c[2])) ? 1.0f : 0.0f;
    var = dnv_prepare_noise(Z, p);
}

// The prefilter's taps g = {1/4, 1/2, 1/4} by offset -1 .. 1.
KHD float dnv_g(int k) { return k == 0 ? 0.5f : 0.25f; }

// The trimmed 3 x 3 prefilter of the variance at (x, y), spacing 1: the Gaussian over the known
// taps inside the image without the first tap holding the largest variance (when two or more are
// known).  The tap is left out, never subtracted.  Returns kbar, and vbar through the reference.
KHD bool dnv_prefilter(const DnParams& P, int x, int y, const DnVar* __restrict__ V, float& vbar) {
    float tv[9];
    bool tk[9];
    int cnt = 0, best = -1;
    float bestv = 0.0f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int k = (dy + 1) * 3 + (dx + 1);
            const uint32_t yy = (uint32_t)y + (uint32_t)dy, xx = (uint32_t)x + (uint32_t)dx;
            tv[k] = 0.0f;
            tk[k] = false;
            if (yy >= P.H || xx >= P.W) continue;
            const DnVar q = V[(size_t)yy * P.W + (size_t)xx];   // both halves used at once: one 64-bit load
            const bool kn = q.known != 0.0f;
            tv[k] = q.v;
            tk[k] = kn;
            cnt += kn ? 1 : 0;
            if (kn && (best < 0 || q.v > bestv)) {
                best = k;
                bestv = q.v;
            }
        }
    if (cnt < 2) best = -1;   // a single known tap is kept
    float gs = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int k = (dy + 1) * 3 + (dx + 1);
            if (!tk[k] || k == best) continue;
            const float g = dnv_g(dy) * dnv_g(dx);
            gs = gs + g * tv[k];
            gw = gw + g;
        }
    const bool kbar = gw > 0.0f;
    vbar = kbar ? gs / gw : 0.0f;
    return kbar;
}

// One iteration at step s for pixel (x, y): reads the records of the previous iteration,
// returns the new colour record and, through rv, the new variance record.
template <bool PREFILTER>
KHD DnRec dnv_filter(const DnParams& P, float floor, int x, int y, int s, const DnRec* __restrict__ G0,
                     const DnRec* __restrict__ G1, const DnRec* __restrict__ C, const DnVar* __restrict__ V, DnVar& rv) {
    const size_t p = (size_t)y * P.W + (size_t)x;
    const bool use0 = (P.on & (DN_NORMAL | DN_DEPTH)) != 0, use1 = (P.on & (DN_TANGENT | DN_COVERAGE)) != 0;
    const DnRec cp = C[p];
    const DnVar vp = V[p];
    DnRec a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0;
    if (use0) a0 = G0[p];
    if (use1) a1 = G1[p];
    bool colour_term = (P.on & DN_COLOR) && cp.w != 0.0f;
    float icv = 0.0f;
    if (colour_term) {   // the prefiltered variance is used by the colour term alone
        float vbar = vp.v;
        const bool kbar = PREFILTER ? dnv_prefilter(P, x, y, V, vbar) : vp.known != 0.0f;
        colour_term = kbar;
        if (kbar) icv = P.inv_sc / (vbar + floor);
    }
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, ws = 0.0f, va = 0.0f, wk = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const uint32_t yy = (uint32_t)y + (uint32_t)(dy * s);   // below 0 wraps past H (H <= 2^31)
        if (yy >= P.H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const uint32_t xx = (uint32_t)x + (uint32_t)(dx * s);
            if (xx >= P.W) continue;
            const size_t q = (size_t)yy * P.W + (size_t)xx;
            const DnRec cq = C[q];
            const DnVar vq = V[q];
            DnRec b0 = a0, b1 = a1;   // the loads together: none waits for another
            if (use0) b0 = G0[q];
            if (use1) b1 = G1[q];
            if (cq.w == 0.0f) continue;   // a tap that is not finite takes no part
            float X = 0.0f;
            if (colour_term) X = X + dn_d2(cp.x, cp.y, cp.z, cq.x, cq.y, cq.z) * icv;
            if (P.on & DN_NORMAL) X = X + dn_d2(a0.x, a0.y, a0.z, b0.x, b0.y, b0.z) * P.inv_sn;
            if (P.on & DN_TANGENT) X = X + dn_d2(a1.x, a1.y, a1.z, b1.x, b1.y, b1.z) * P.inv_st;
            if (P.on & DN_DEPTH) { const float e = a0.w - b0.w; X = X + (e * e) * P.inv_sd; }
            if (P.on & DN_COVERAGE) { const float e = a1.w - b1.w; X = X + (e * e) * P.inv_sv; }
            const float w = (dn_h(dy) * dn_h(dx)) * k_expf(-X);
            if (w > 0.0f) {   // a NaN weight fails the comparison
                ar = ar + w * cq.x;
                ag = ag + w * cq.y;
                ab = ab + w * cq.z;
                ws = ws + w;
                if (vq.known != 0.0f) {
                    va = va + (w * w) * vq.v;
                    wk = wk + w;
                }
            }
        }
    }
    DnRec r = cp;   // no tap counted: the bits as they are, the variance record too
    rv = vp;
    if (ws > 0.0f) {
        r.x = ar / ws;
        r.y = ag / ws;
        r.z = ab / ws;
        r.w = (dn_finite(r.x) && dn_finite(r.y) && dn_finite(r.z)) ? 1.0f : 0.0f;
        const bool known = wk > 0.0f;
        rv.v = known ? va / (wk * wk) : 0.0f;
        rv.known = known ? 1.0f : 0.0f;
    }
    return r;
}

KHD float dnv_finish_variance(const DnVar& v) { return v.known != 0.0f ? v.v : k_inf(); }

// ---- the argument checks of both entries (host code) -------------------------------------------
// nullptr: accepted, and P / G / Z are filled in (Z.mom and Z.mean are the device entry's to set);
// otherwise the cause, with its status in st.
inline const char* dnv_check(const khp_denoise_params* p, const float* colour, const khp_aov_buffers* g,
                             const khp_denoise_noise* noise, const float* out, bool host_entry, DnParams& P, DnPlanes& G,
                             DnvNoise& Z, khp_status& st) {
    st = KHP_EINVAL;
    if (!noise) return "noise is null";
    if (noise->source > KHP_NOISE_CONTEXT) return "noise: unknown source (KHP_NOISE_*)";
    if (noise->prefilter > 1u) return "noise: prefilter must be 0 or 1";
    if (noise->reserved != 0u) return "noise: reserved must be 0";
    if (!dn_finite(noise->floor) || noise->floor < 0.0f) return "noise: floor must be finite and >= 0";
    if (noise->source == KHP_NOISE_PLANE && !noise->variance) return "noise: KHP_NOISE_PLANE needs the variance plane";
    if (noise->source == KHP_NOISE_MOMENTS && (!noise->m2 || !noise->count))
        return "noise: KHP_NOISE_MOMENTS needs the m2 and count planes";
    if (host_entry && noise->source == KHP_NOISE_CONTEXT)
        return "noise: KHP_NOISE_CONTEXT does not apply to khp_denoise_var_host, which has no context";
    if (p && (p->flags & KHP_DENOISE_DEMODULATE)) {
        st = KHP_EUNSUPPORTED;
        return "KHP_DENOISE_DEMODULATE: a scalar variance has no per-channel albedo division";
    }
    if (const char* why = dn_check(p, colour, g, out, host_entry, P, G)) return why;
    Z.source = noise->source;
    Z.prefilter = noise->prefilter;
    Z.floor = noise->floor;
    Z.variance = noise->source == KHP_NOISE_PLANE ? noise->variance : nullptr;
    Z.m2 = noise->source == KHP_NOISE_MOMENTS ? noise->m2 : nullptr;
    Z.count = noise->source == KHP_NOISE_MOMENTS ? noise->count : nullptr;
    Z.mom = nullptr;
    Z.mean = nullptr;
    Z.out_variance = noise->out_variance;
    return nullptr;
}

}  // namespace khp
