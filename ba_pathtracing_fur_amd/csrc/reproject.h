// reproject.h -- the definition of khp_reproject / khp_reproject_host (kirk_hip.h,
// DESIGN.md §18): carry the previous camera's frame into the current camera's
// pixels and blend the current frame into it.
//
// Everything that computes a value is a KHD function in this header, compiled
// into the host entry (reproject_host.cpp, g++) and into the gfx950 kernel
// (reproject_dev.h, included by render.hip).  Every operation is one float32
// operation in the order written; both sides build with -ffp-contract=off, so
// the two entries give the same bits, and tests/_reprojectref.py restates the same
// sequence in numpy.  No atomics and no order that depends on scheduling: a
// pixel's outputs are a function of the two frames alone.
//
// Four steps per pixel, all in rp_pixel:
//   locate   the pixel centre's ray of the current camera, and on it the surface
//            point at depth / coverage (a direction, a point at infinity, for a
//            background pixel);
//   project  that point through the history camera: a continuous pixel position
//            (fx, fy), the motion vector, and whether the projection exists;
//   taps     the four bilinear taps of the history around (fx, fy), each counted
//            only if it is inside, finite, has a history length and passes the
//            enabled depth / normal / tangent / coverage / object tests;
//   blend    history h of effective length N with the current colour c of weight s:
//            h + (s / (N + s)) (c - h), length N + s, the variance propagated with
//            the squared weights; the current frame alone where no tap counted.
// The argument checks of both entries are rp_check.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kirk_hip.h"
#include "denoise.h"
#include "kmath.h"

namespace khp {

enum : uint32_t { RP_DEPTH = 1u, RP_NORMAL = 2u, RP_TANGENT = 4u, RP_COVERAGE = 8u, RP_OBJECT = 16u, RP_HIST = 32u };

// The parameters as rp_pixel uses them.
struct RpParams {
    uint32_t W, H;
    uint32_t on;   // RP_* bits: the enabled tests, and whether there is a history frame
    float samples, max_history;
    float tol_d, tol_n, tol_t, tol_c;
};

// One frame's camera and planes (host or device memory, as the entry says).  rp_check
// leaves a pointer null unless rp_pixel reads the plane: "non-null" is "read".
struct RpFrame {
    khp_camera cam;
    const float* colour;
    const float* variance;
    const float* length;
    const float* normal;
    const float* tangent;
    const float* depth;
    const float* coverage;
    const int32_t* object;
};

struct RpOut {
    float* colour;
    float* length;
    float* variance;
    float* motion;
};

// The history planes that need the history's coverage: the depth and the unit vectors divide by it.
KHD bool rp_hist_reads_coverage(uint32_t on) { return (on & (RP_DEPTH | RP_NORMAL | RP_TANGENT | RP_COVERAGE)) != 0; }
// A variance is known when it is finite and not negative.
KHD bool rp_known(float v) { return dn_finite(v) && v >= 0.0f; }

// dn_unit's operations, and whether the vector has a length.
KHD bool rp_unit(const float* v, float inv, float& ox, float& oy, float& oz) {
    dn_unit(v, inv, ox, oy, oz);
    return ox != 0.0f || oy != 0.0f || oz != 0.0f;
}

// One pixel: reads the two frames, writes the outputs that are not null.
KHD void rp_pixel(const RpParams& P, const RpFrame& C, const RpFrame& Hs, const RpOut& O, uint32_t x, uint32_t y) {
    const size_t p = (size_t)y * P.W + (size_t)x;
    const float unknown = k_inf();

    // ---- locate ----
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const float sx = px * C.cam.pixel_size, sy = py * C.cam.pixel_size;
    const v3 pos = ld3(C.cam.position);
    const v3 dir = ((ld3(C.cam.bottom_left) + ld3(C.cam.axis_x) * sx) + ld3(C.cam.axis_y) * sy) - pos;
    const v3 u = dir / sqrtf((dir.x * dir.x + dir.y * dir.y) + dir.z * dir.z);
    const float cv = C.coverage[p];
    // the current frame's other per-pixel loads are issued here too, ahead of the first use and of every
    // store (an output may be the current colour or variance: the pixel is read before it is written)
    const float c0 = C.colour[3 * p], c1 = C.colour[3 * p + 1], c2 = C.colour[3 * p + 2];
    const float vc = C.variance ? C.variance[p] : -1.0f;
    const float dp = C.depth[p];
    const bool surf = cv > 0.0f;
    const float inv_cv = surf ? 1.0f / cv : 0.0f;
    const float d = surf ? dp * inv_cv : 0.0f;

    // ---- project ----
    float fx = 0.0f, fy = 0.0f, dist = 0.0f;
    bool exists = false;
    if (P.on & RP_HIST) {
        const v3 hpos = ld3(Hs.cam.position), hax = ld3(Hs.cam.axis_x), hay = ld3(Hs.cam.axis_y);
        v3 w = u;
        if (surf) {
            w = (pos + u * d) - hpos;
            dist = sqrtf(dot(w, w));
        }
        const v3 n = cross(hax, hay);
        const float det = dot(w, n);
        const v3 e = ld3(Hs.cam.bottom_left) - hpos;
        const float t = dot(e, n) / det;
        const v3 hvec = w * t - e;
        const float a = dot(hvec, hax) / dot(hax, hax), b = dot(hvec, hay) / dot(hay, hay);
        fx = a / Hs.cam.pixel_size;
        fy = b / Hs.cam.pixel_size;
        exists = dn_finite(det) && det != 0.0f && dn_finite(t) && t > 0.0f;
    }
    const float mx = exists ? fx - px : k_nan(), my = exists ? fy - py : k_nan();

    // ---- taps ----
    float ws = 0.0f, ac0 = 0.0f, ac1 = 0.0f, ac2 = 0.0f, al = 0.0f, va = 0.0f, wk = 0.0f;
    const float gx = fx - 0.5f, gy = fy - 0.5f;
    const bool cand = exists && gx > -1.0f && gx < (float)P.W && gy > -1.0f && gy < (float)P.H;   // a NaN fails
    if (cand) {
        const float x0f = floorf(gx), y0f = floorf(gy);
        const float wx = gx - x0f, wy = gy - y0f;
        const int64_t x0 = (int64_t)x0f, y0 = (int64_t)y0f;   // checked above: -1 .. 2^31
        float an0 = 0.0f, an1 = 0.0f, an2 = 0.0f, at0 = 0.0f, at1 = 0.0f, at2 = 0.0f;
        bool has_n = false, has_t = false;
        if (P.on & RP_NORMAL) has_n = rp_unit(C.normal + 3 * p, inv_cv, an0, an1, an2);
        if (P.on & RP_TANGENT) has_t = rp_unit(C.tangent + 3 * p, inv_cv, at0, at1, at2);
        const int32_t obj = (P.on & RP_OBJECT) ? C.object[p] : 0;
        // the four taps' loads first, together: none waits for another.  A tap outside the
        // image reads the nearest pixel inside (and is not counted).
        bool inside[4];
        float qc[4][3], ql[4], qv[4], qcv[4], qd[4], qn[4][3], qt[4][3];
        int32_t qo[4];
        for (int k = 0; k < 4; ++k) {
            const int64_t xq = x0 + (k & 1), yq = y0 + (k >> 1);
            inside[k] = xq >= 0 && xq < (int64_t)P.W && yq >= 0 && yq < (int64_t)P.H;
            const int64_t xc = xq < 0 ? 0 : (xq >= (int64_t)P.W ? (int64_t)P.W - 1 : xq);
            const int64_t yc = yq < 0 ? 0 : (yq >= (int64_t)P.H ? (int64_t)P.H - 1 : yq);
            const size_t q = (size_t)yc * P.W + (size_t)xc;
            qc[k][0] = Hs.colour[3 * q];
            qc[k][1] = Hs.colour[3 * q + 1];
            qc[k][2] = Hs.colour[3 * q + 2];
            ql[k] = Hs.length[q];
            qv[k] = Hs.variance ? Hs.variance[q] : -1.0f;
            qcv[k] = Hs.coverage ? Hs.coverage[q] : 0.0f;
            qd[k] = Hs.depth ? Hs.depth[q] : 0.0f;
            for (int i = 0; i < 3; ++i) {
                qn[k][i] = Hs.normal ? Hs.normal[3 * q + i] : 0.0f;
                qt[k][i] = Hs.tangent ? Hs.tangent[3 * q + i] : 0.0f;
            }
            qo[k] = Hs.object ? Hs.object[q] : 0;
        }
        for (int k = 0; k < 4; ++k) {   // dy outer, dx inner
            const float bw = ((k >> 1) ? wy : 1.0f - wy) * ((k & 1) ? wx : 1.0f - wx);
            bool ok = inside[k] && bw > 0.0f && dn_finite(qc[k][0]) && dn_finite(qc[k][1]) && dn_finite(qc[k][2]) &&
                      dn_finite(ql[k]) && ql[k] > 0.0f;
            const bool surf_q = qcv[k] > 0.0f;
            const float inv_q = surf_q ? 1.0f / qcv[k] : 0.0f;
            if (P.on & RP_DEPTH) {
                ok = ok && surf == surf_q;
                if (surf && surf_q) {
                    const float dq = qd[k] * inv_q;
                    ok = ok && fabsf(dq - dist) <= P.tol_d * dist;   // a NaN rejects
                }
            }
            if (P.on & RP_NORMAL) {
                float b0, b1, b2;
                const bool has_q = rp_unit(qn[k], inv_q, b0, b1, b2);
                if (has_n && has_q) ok = ok && 1.0f - ((an0 * b0 + an1 * b1) + an2 * b2) <= P.tol_n;
            }
            if (P.on & RP_TANGENT) {
                float b0, b1, b2;
                const bool has_q = rp_unit(qt[k], inv_q, b0, b1, b2);
                if (has_t && has_q) ok = ok && 1.0f - ((at0 * b0 + at1 * b1) + at2 * b2) <= P.tol_t;
            }
            if (P.on & RP_COVERAGE) ok = ok && fabsf(cv - qcv[k]) <= P.tol_c;
            if (P.on & RP_OBJECT) ok = ok && obj == qo[k];
            if (ok) {
                ws = ws + bw;
                ac0 = ac0 + bw * qc[k][0];
                ac1 = ac1 + bw * qc[k][1];
                ac2 = ac2 + bw * qc[k][2];
                al = al + bw * ql[k];
                if (rp_known(qv[k])) {
                    va = va + (bw * bw) * qv[k];
                    wk = wk + bw;
                }
            }
        }
    }
    const bool have = ws > 0.0f;
    const float h0 = ac0 / ws, h1 = ac1 / ws, h2 = ac2 / ws;   // used only with have
    const float N = al / ws;
    const bool vh_known = wk > 0.0f;
    const float vh = va / (wk * wk);

    // ---- blend ----
    const bool fin = dn_finite(c0) && dn_finite(c1) && dn_finite(c2);
    const bool vc_known = rp_known(vc);
    const float s = P.samples;
    const float Nc = P.max_history > 0.0f ? gmin(N, P.max_history) : N;
    float r0 = c0, r1 = c1, r2 = c2, len = 0.0f, var = unknown;   // !have && !fin: the bits as they are
    if (have && fin) {
        const float alpha = s / (Nc + s);
        r0 = h0 + alpha * (c0 - h0);
        r1 = h1 + alpha * (c1 - h1);
        r2 = h2 + alpha * (c2 - h2);
        len = Nc + s;
        if (vc_known) {
            const float om = 1.0f - alpha;
            var = vh_known ? (om * om) * vh + (alpha * alpha) * vc : vc;
        }
    } else if (have) {   // the history repairs the dead pixel
        r0 = h0;
        r1 = h1;
        r2 = h2;
        len = Nc;
        if (vh_known) var = vh;
    } else if (fin) {    // disocclusion: the current frame alone
        len = s;
        if (vc_known) var = vc;
    }
    if (O.motion) {
        O.motion[2 * p] = mx;
        O.motion[2 * p + 1] = my;
    }
    if (O.colour) {
        O.colour[3 * p] = r0;
        O.colour[3 * p + 1] = r1;
        O.colour[3 * p + 2] = r2;
    }
    if (O.length) O.length[p] = len;
    if (O.variance) O.variance[p] = var;
}

// ---- the argument checks of both entries (host code) -------------------------------------------
// nullptr: accepted, and P / C / Hs / O are filled in; otherwise the cause, for KHP_EINVAL.
inline const char* rp_check(const khp_reproject_params* p, const khp_reproject_frame* cur, const khp_reproject_frame* hist,
                            const khp_reproject_out* out, bool host_entry, RpParams& P, RpFrame& C, RpFrame& Hs, RpOut& O) {
    if (!p || !cur || !out) return "null argument";
    const uint64_t npix = (uint64_t)p->width * p->height;
    if (npix == 0) return "width * height must be > 0";
    if (npix > (1ull << 31)) return "image too large: width * height above 2^31";
    if (p->flags & ~(uint32_t)(KHP_REPROJECT_DEVICE | KHP_REPROJECT_MATCH_OBJECT)) return "flags: unknown KHP_REPROJECT_* bits";
    if (host_entry && (p->flags & KHP_REPROJECT_DEVICE)) return "flags: KHP_REPROJECT_DEVICE does not apply to khp_reproject_host";
    if (p->reserved[0] || p->reserved[1] || p->reserved[2]) return "reserved must be 0";
    if (cur->reserved || (hist && hist->reserved)) return "reserved must be 0 (a frame's)";
    if (!dn_finite(p->samples) || !(p->samples > 0.0f)) return "samples must be finite and > 0";
    if (!(p->max_history >= 0.0f)) return "max_history must be >= 0 (0: no cap)";
    const float tol[4] = {p->depth_tol, p->normal_tol, p->tangent_tol, p->coverage_tol};
    const char* const tol_bad[4] = {"depth_tol must be >= 0", "normal_tol must be >= 0", "tangent_tol must be >= 0",
                                    "coverage_tol must be >= 0"};
    for (int k = 0; k < 4; ++k)
        if (!(tol[k] >= 0.0f)) return tol_bad[k];   // a NaN fails the comparison
    if (!out->colour && !out->length && !out->variance && !out->motion) return "out: every output is null";
    if (!cur->colour) return "colour is null (the current frame's)";
    if (!cur->aov.depth || !cur->aov.coverage)
        return "the current frame's depth and coverage planes are needed to locate its pixels";
    P.W = p->width;
    P.H = p->height;
    P.on = hist ? RP_HIST : 0u;
    if (hist) {   // without a history frame no test runs and no other plane is read
        P.on |= (p->depth_tol > 0.0f ? RP_DEPTH : 0u) | (p->normal_tol > 0.0f ? RP_NORMAL : 0u) |
                (p->tangent_tol > 0.0f ? RP_TANGENT : 0u) | (p->coverage_tol > 0.0f ? RP_COVERAGE : 0u) |
                ((p->flags & KHP_REPROJECT_MATCH_OBJECT) ? RP_OBJECT : 0u);
        if (!hist->colour) return "colour is null (the history frame's)";
        if (!hist->length) return "length is null: a history frame needs its length plane";
        if ((P.on & RP_DEPTH) && !hist->aov.depth) return "depth_tol > 0 needs the depth plane of both frames";
        if ((P.on & RP_NORMAL) && (!cur->aov.normal || !hist->aov.normal)) return "normal_tol > 0 needs the normal plane of both frames";
        if ((P.on & RP_TANGENT) && (!cur->aov.tangent || !hist->aov.tangent))
            return "tangent_tol > 0 needs the tangent plane of both frames";
        if ((P.on & RP_OBJECT) && (!cur->aov.object || !hist->aov.object))
            return "KHP_REPROJECT_MATCH_OBJECT needs the object plane of both frames";
        if (rp_hist_reads_coverage(P.on) && !hist->aov.coverage)
            return "the history's coverage plane is needed when depth, normal, tangent or coverage is tested";
    }
    P.samples = p->samples;
    P.max_history = p->max_history;
    P.tol_d = p->depth_tol;
    P.tol_n = p->normal_tol;
    P.tol_t = p->tangent_tol;
    P.tol_c = p->coverage_tol;
    C = RpFrame{};
    Hs = RpFrame{};
    C.cam = cur->camera;
    C.colour = cur->colour;
    C.variance = cur->variance;
    C.depth = cur->aov.depth;
    C.coverage = cur->aov.coverage;
    if (P.on & RP_NORMAL) C.normal = cur->aov.normal;
    if (P.on & RP_TANGENT) C.tangent = cur->aov.tangent;
    if (P.on & RP_OBJECT) C.object = cur->aov.object;
    if (hist) {
        Hs.cam = hist->camera;
        Hs.colour = hist->colour;
        Hs.variance = hist->variance;
        Hs.length = hist->length;
        if (P.on & RP_DEPTH) Hs.depth = hist->aov.depth;
        if (rp_hist_reads_coverage(P.on)) Hs.coverage = hist->aov.coverage;
        if (P.on & RP_NORMAL) Hs.normal = hist->aov.normal;
        if (P.on & RP_TANGENT) Hs.tangent = hist->aov.tangent;
        if (P.on & RP_OBJECT) Hs.object = hist->aov.object;
        // the history is gathered: an output written over it would be read by other pixels
        const void* const hp[8] = {Hs.colour, Hs.variance, Hs.length, Hs.depth, Hs.coverage, Hs.normal, Hs.tangent, Hs.object};
        const void* const op[4] = {out->colour, out->length, out->variance, out->motion};
        for (const void* o : op)
            for (const void* h : hp)
                if (o && o == h) return "an output is a plane of the history frame: the history is gathered, not read per pixel";
    }
    O.colour = out->colour;
    O.length = out->length;
    O.variance = out->variance;
    O.motion = out->motion;
    return nullptr;
}

}  // namespace khp
