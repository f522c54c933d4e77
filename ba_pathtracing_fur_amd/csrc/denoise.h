// denoise.h -- the definition of khp_denoise / khp_denoise_host (kirk_hip.h,
// DESIGN.md §13): a guided a-trous filter over the planes khp_render_aov writes.
//
// Everything that computes a value is a KHD function in this header, compiled
// into the host entry (denoise_host.cpp, g++) and into the gfx950 kernels
// (denoise_dev.h, included by render.hip).  Every operation is one float32
// operation in the order written; both sides build with -ffp-contract=off, so
// the two entries give the same bits, and tests/_denoiseref.py restates the same
// sequence in numpy.  No atomics and no order that depends on scheduling: a
// pixel's new colour is a function of the previous iteration's records alone.
//
// Three stages:
//   dn_prepare  per pixel, three 16-byte records: (n.xyz, d), (t.xyz, cv), (c.rgb, fin)
//               and, demodulating, (m.rgb, 0);
//   dn_filter   one iteration for one pixel: the 25 taps, dy outer, dx inner;
//   dn_finish   with DEMODULATE c * m.
// The argument checks of both entries are dn_check.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kirk_hip.h"
#include "kmath.h"

namespace khp {

// One 16-byte record; every load of one is a single aligned 128-bit load.
struct alignas(16) DnRec {
    float x, y, z, w;
};

enum : uint32_t { DN_COLOR = 1u, DN_NORMAL = 2u, DN_TANGENT = 4u, DN_DEPTH = 8u, DN_COVERAGE = 16u, DN_DEMOD = 32u };

// The parameters as the stages use them: which terms are on and 1.0f / (s * s) of each.
struct DnParams {
    uint32_t W, H;
    uint32_t on;     // DN_* bits
    float inv_sc, inv_sn, inv_st, inv_sd, inv_sv;
    float clamp;
};

// The caller's planes (host or device memory, as the entry says).
struct DnPlanes {
    const float* colour;
    const float* normal;
    const float* albedo;
    const float* tangent;
    const float* depth;
    const float* coverage;
};

KHD bool dn_finite(float x) { return (bits_from_f(x) & 0x7f800000u) != 0x7f800000u; }
KHD float dn_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float ex = ax - bx, ey = ay - by, ez = az - bz;
    return (ex * ex + ey * ey) + ez * ez;
}

// The B3 spline taps h = {1/16, 1/4, 3/8, 1/4, 1/16} by offset -2 .. 2.
KHD float dn_h(int k) { return k == 0 ? 0.375f : ((k == 1 || k == -1) ? 0.25f : 0.0625f); }

// v * inv per component, then divided by its length; 0 where it has none (or the length is NaN).
KHD void dn_unit(const float* v, float inv, float& ox, float& oy, float& oz) {
    const float x = v[0] * inv, y = v[1] * inv, z = v[2] * inv;
    const float l = sqrtf((x * x + y * y) + z * z);
    const bool has = l > 0.0f;
    ox = has ? x / l : 0.0f;
    oy = has ? y / l : 0.0f;
    oz = has ? z / l : 0.0f;
}

// Which planes the call reads.
KHD bool dn_reads_coverage(uint32_t on) { return (on & (DN_NORMAL | DN_TANGENT | DN_DEPTH | DN_COVERAGE | DN_DEMOD)) != 0; }

KHD void dn_prepare(const DnParams& P, const DnPlanes& G, size_t p, DnRec& g0, DnRec& g1, DnRec& col, DnRec& mod) {
    const float cv = dn_reads_coverage(P.on) ? G.coverage[p] : 0.0f;
    const float inv = cv > 0.0f ? 1.0f / cv : 0.0f;
    g0.x = g0.y = g0.z = g0.w = 0.0f;
    g1.x = g1.y = g1.z = 0.0f;
    g1.w = cv;
    if (P.on & DN_NORMAL) dn_unit(G.normal + 3 * p, inv, g0.x, g0.y, g0.z);
    if (P.on & DN_TANGENT) dn_unit(G.tangent + 3 * p, inv, g1.x, g1.y, g1.z);
    if (P.on & DN_DEPTH) g0.w = G.depth[p] * inv;
    float c[3] = {G.colour[3 * p], G.colour[3 * p + 1], G.colour[3 * p + 2]};
    if (P.clamp > 0.0f)
        for (int k = 0; k < 3; ++k) c[k] = c[k] > P.clamp ? P.clamp : c[k];   // NaN and -inf pass
    mod.x = mod.y = mod.z = 1.0f;
    mod.w = 0.0f;
    if (P.on & DN_DEMOD) {
        const float rest = 1.0f - cv;
        mod.x = gmax(G.albedo[3 * p] + rest, 1e-3f);
        mod.y = gmax(G.albedo[3 * p + 1] + rest, 1e-3f);
        mod.z = gmax(G.albedo[3 * p + 2] + rest, 1e-3f);
        c[0] = c[0] / mod.x;
        c[1] = c[1] / mod.y;
        c[2] = c[2] / mod.z;
    }
    col.x = c[0];
    col.y = c[1];
    col.z = c[2];
    col.w = (dn_finite(c[0]) && dn_finite(c[1]) && dn_finite(c[2])) ? 1.0f : 0.0f;
}

// One iteration at step s for pixel (x, y): reads the records of the previous
// iteration, returns the new colour record.
KHD DnRec dn_filter(const DnParams& P, int x, int y, int s, const DnRec* __restrict__ G0, const DnRec* __restrict__ G1,
                    const DnRec* __restrict__ C) {
    const size_t p = (size_t)y * P.W + (size_t)x;
    const bool use0 = (P.on & (DN_NORMAL | DN_DEPTH)) != 0, use1 = (P.on & (DN_TANGENT | DN_COVERAGE)) != 0;
    const DnRec cp = C[p];
    DnRec a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0;
    if (use0) a0 = G0[p];
    if (use1) a1 = G1[p];
    const bool colour_term = (P.on & DN_COLOR) && cp.w != 0.0f;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, ws = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const uint32_t yy = (uint32_t)y + (uint32_t)(dy * s);   // below 0 wraps past H (H <= 2^31)
        if (yy >= P.H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const uint32_t xx = (uint32_t)x + (uint32_t)(dx * s);
            if (xx >= P.W) continue;
            const size_t q = (size_t)yy * P.W + (size_t)xx;
            const DnRec cq = C[q];
            DnRec b0 = a0, b1 = a1;   // the three loads together: none waits for another
            if (use0) b0 = G0[q];
            if (use1) b1 = G1[q];
            if (cq.w == 0.0f) continue;   // a tap that is not finite takes no part
            float X = 0.0f;
            if (colour_term) X = X + dn_d2(cp.x, cp.y, cp.z, cq.x, cq.y, cq.z) * P.inv_sc;
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
            }
        }
    }
    DnRec r = cp;   // no tap counted: the bits as they are
    if (ws > 0.0f) {
        r.x = ar / ws;
        r.y = ag / ws;
        r.z = ab / ws;
        r.w = (dn_finite(r.x) && dn_finite(r.y) && dn_finite(r.z)) ? 1.0f : 0.0f;
    }
    return r;
}

KHD void dn_finish(const DnParams& P, const DnRec& c, const DnRec& mod, float* out3) {
    if (P.on & DN_DEMOD) {
        out3[0] = c.x * mod.x;
        out3[1] = c.y * mod.y;
        out3[2] = c.z * mod.z;
    } else {
        out3[0] = c.x;
        out3[1] = c.y;
        out3[2] = c.z;
    }
}

// ---- the argument checks of both entries (host code) -------------------------------------------
// nullptr: accepted, and P / G are filled in; otherwise the cause, for KHP_EINVAL.
inline const char* dn_check(const khp_denoise_params* p, const float* colour, const khp_aov_buffers* g, const float* out,
                            bool host_entry, DnParams& P, DnPlanes& G) {
    if (!p || !g || !out) return "null argument";
    if (host_entry && !colour) return "colour is null: khp_denoise_host has no framebuffer to filter";
    const uint64_t npix = (uint64_t)p->width * p->height;
    if (npix == 0) return "width * height must be > 0";
    if (npix > (1ull << 31)) return "image too large: width * height above 2^31";
    if (p->iterations < 1 || p->iterations > 8) return "iterations must be 1..8";
    if (p->flags & ~(uint32_t)(KHP_DENOISE_DEVICE | KHP_DENOISE_DEMODULATE)) return "flags: unknown KHP_DENOISE_* bits";
    if (host_entry && (p->flags & KHP_DENOISE_DEVICE)) return "flags: KHP_DENOISE_DEVICE does not apply to khp_denoise_host";
    if (p->reserved[0] || p->reserved[1]) return "reserved must be 0";
    const float sig[5] = {p->sigma_color, p->sigma_normal, p->sigma_tangent, p->sigma_depth, p->sigma_coverage};
    const char* const sig_bad[5] = {"sigma_color must be finite and >= 0", "sigma_normal must be finite and >= 0",
                                    "sigma_tangent must be finite and >= 0", "sigma_depth must be finite and >= 0",
                                    "sigma_coverage must be finite and >= 0"};
    for (int k = 0; k < 5; ++k)
        if (!dn_finite(sig[k]) || sig[k] < 0.0f) return sig_bad[k];
    if (!dn_finite(p->clamp) || p->clamp < 0.0f) return "clamp must be finite and >= 0";
    if (p->sigma_normal > 0.0f && !g->normal) return "sigma_normal > 0 needs the normal plane";
    if (p->sigma_tangent > 0.0f && !g->tangent) return "sigma_tangent > 0 needs the tangent plane";
    if (p->sigma_depth > 0.0f && !g->depth) return "sigma_depth > 0 needs the depth plane";
    if (p->sigma_coverage > 0.0f && !g->coverage) return "sigma_coverage > 0 needs the coverage plane";
    const bool demod = (p->flags & KHP_DENOISE_DEMODULATE) != 0;
    if (demod && !g->albedo) return "KHP_DENOISE_DEMODULATE needs the albedo plane";
    P.W = p->width;
    P.H = p->height;
    P.on = (p->sigma_color > 0.0f ? DN_COLOR : 0u) | (p->sigma_normal > 0.0f ? DN_NORMAL : 0u) |
           (p->sigma_tangent > 0.0f ? DN_TANGENT : 0u) | (p->sigma_depth > 0.0f ? DN_DEPTH : 0u) |
           (p->sigma_coverage > 0.0f ? DN_COVERAGE : 0u) | (demod ? DN_DEMOD : 0u);
    if (dn_reads_coverage(P.on) && !g->coverage)
        return "the coverage plane is needed when normal, tangent, depth or albedo is used";
    auto inv = [](float s) { return s > 0.0f ? 1.0f / (s * s) : 0.0f; };
    P.inv_sc = inv(p->sigma_color);
    P.inv_sn = inv(p->sigma_normal);
    P.inv_st = inv(p->sigma_tangent);
    P.inv_sd = inv(p->sigma_depth);
    P.inv_sv = inv(p->sigma_coverage);
    P.clamp = p->clamp;
    G.colour = colour;
    G.normal = g->normal;
    G.albedo = g->albedo;
    G.tangent = g->tangent;
    G.depth = g->depth;
    G.coverage = g->coverage;
    return nullptr;
}

}  // namespace khp
