// moments_dev.h -- the per-pixel sample moments on the device: the kernels, the state's
// lifecycle and the entries (included last by render.hip, so that every other kernel
// keeps its place in the code object).  Definition: moments.h and DESIGN.md §14.
//
// The state (khp_ctx::mom) is two MomRec per image pixel, (mean.rgb, n) and (m2.rgb, bad).
// It is folded by k_accumulate_m / k_accumulate_all_m, which launch_accumulate /
// launch_accumulate_all (render.hip) pick while khp_ctx::moments_on is set: every
// schedule ends in those launches, so none has a case of its own here.  Both are instances
// of the accumulate bodies of render.hip (fold_sample, accumulate_frame, accumulate_all),
// which hold the one definition of the running mean and of the fold beside it.
//
//   k_accumulate_m      accumulate_frame<true, true>: one frame per launch, a lane per owned pixel;
//   k_accumulate_all_m  accumulate_all<true>: every fused frame in one launch, the samples staged
//                       through LDS: a thread loads its pixel's two records once and stores them once;
//   k_moments_read      a lane per pixel: the two records -> whichever planes were asked
//                       for, and rel_error from mom_rel_error.
#pragma once

#include "moments.h"

// Launched in place of k_accumulate and k_accumulate_all while khp_set_moments is on: the same
// bodies (render.hip: accumulate_frame, accumulate_all), compiled with the moments fold beside the
// running mean.
__global__ __launch_bounds__(256) void k_accumulate_m(Wave Wv, float* fb, uint32_t fr, MomRec* st) {
    accumulate_frame<true, true>(Wv, fb, fr, st);
}
__global__ __launch_bounds__(ACC_PIX) void k_accumulate_all_m(Wave Wv, float* fb, MomRec* st) {
    accumulate_all<true>(Wv, fb, st);
}

__global__ __launch_bounds__(256) void k_moments_read(const MomRec* __restrict__ st, uint64_t npix, khp_moments_buffers out) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const MomRec a = st[2 * p], b = st[2 * p + 1];
    if (out.mean) {
        out.mean[3 * p] = a.x; out.mean[3 * p + 1] = a.y; out.mean[3 * p + 2] = a.z;
    }
    if (out.m2) {
        out.m2[3 * p] = b.x; out.m2[3 * p + 1] = b.y; out.m2[3 * p + 2] = b.z;
    }
    if (out.count) out.count[p] = a.w;
    if (out.bad) out.bad[p] = b.w;
    if (out.rel_error) out.rel_error[p] = mom_rel_error(a, b);
}

// ---- host side ---------------------------------------------------------------------------
// A zeroed state for a framebuffer of npix pixels, queued on the context's stream.
static khp_status moments_remake(khp_ctx* c, size_t npix) {
    const size_t bytes = 2 * npix * sizeof(MomRec);
    if (c->mom.ensure(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KHP_ENOMEM, "khp_set_moments: no device memory for 32 bytes per pixel");
    }
    HIPCHK(hipMemsetAsync(c->mom.p, 0, bytes, c->stream));
    return KHP_OK;
}

extern "C" khp_status khp_get_moments(khp_ctx* c, khp_moments* out) {
    if (!c || !out) return fail(KHP_EINVAL, "null argument");
    *out = khp_moments{};
    out->enabled = c->moments_on ? 1u : 0u;
    return KHP_OK;
}

extern "C" khp_status khp_set_moments(khp_ctx* c, const khp_moments* m) {
    if (!c || !m) return fail(KHP_EINVAL, "null argument");
    if (m->enabled > 1u) return fail(KHP_EINVAL, "khp_set_moments: enabled must be 0 or 1");
    if (m->reserved[0] != 0u || m->reserved[1] != 0u || m->reserved[2] != 0u)
        return fail(KHP_EINVAL, "khp_set_moments: reserved must be 0");
    const bool on = m->enabled != 0u;
    if (on == c->moments_on) return KHP_OK;
    HIPCHK(hipSetDevice(c->device));
    KHPCHK(drain(c));   // frames in flight finish with the accumulator they started with
    if (on && c->fb.p) {
        KHPCHK(moments_remake(c, (size_t)c->fbW * c->fbH));
        KHPCHK(wait_stream(c, c->stream, "the moments state"));
    }
    if (!on) {
        c->mom.release();
        c->mom_stage.release();
    }
    c->moments_on = on;
    return KHP_OK;
}

extern "C" khp_status khp_read_moments(khp_ctx* c, uint32_t flags, const khp_moments_buffers* out) {
    // the arguments first, then the context
    if (!c || !out) return fail(KHP_EINVAL, "null argument");
    if (flags & ~KHP_MOMENTS_DEVICE) return fail(KHP_EINVAL, "khp_read_moments: unknown flag");
    if (!out->mean && !out->m2 && !out->count && !out->bad && !out->rel_error)
        return fail(KHP_EINVAL, "khp_read_moments: every plane is NULL");
    KHPCHK(drain(c));   // complete asynchronous frames first, as khp_read_framebuffer does
    if (!c->moments_on) return fail(KHP_ENOTREADY, "khp_read_moments: moments are off (khp_set_moments first)");
    if (!c->fb.p || !c->mom.p) return fail(KHP_ENOTREADY, "nothing rendered yet");
    HIPCHK(hipSetDevice(c->device));
    const bool on_device = (flags & KHP_MOMENTS_DEVICE) != 0;
    const size_t npix = (size_t)c->fbW * c->fbH;
    // the planes in struct order, with their 4-byte words per pixel
    struct Plane { void* host; size_t k; void* dev; };
    Plane pl[5] = {{out->mean, 3, nullptr}, {out->m2, 3, nullptr}, {out->count, 1, nullptr},
                   {out->bad, 1, nullptr}, {out->rel_error, 1, nullptr}};
    if (on_device) {   // a host pointer here would be written by a kernel
        for (Plane& q : pl) {
            if (q.host && !is_device_ptr(q.host))
                return fail(KHP_EINVAL, "KHP_MOMENTS_DEVICE: a plane is not device memory");
            q.dev = q.host;
        }
    } else {           // host buffers go through the staging area
        size_t words = 0;
        for (const Plane& q : pl)
            if (q.host) words += q.k * npix;
        if (c->mom_stage.ensure(words * 4) != hipSuccess) {
            (void)hipGetLastError();
            return fail(KHP_ENOMEM, "khp_read_moments: no device memory for the staging area");
        }
        uint32_t* at = c->mom_stage.as<uint32_t>();
        for (Plane& q : pl) {
            if (!q.host) continue;
            q.dev = at;
            at += q.k * npix;
        }
    }
    khp_moments_buffers D;
    D.mean = (float*)pl[0].dev;
    D.m2 = (float*)pl[1].dev;
    D.count = (uint32_t*)pl[2].dev;
    D.bad = (uint32_t*)pl[3].dev;
    D.rel_error = (float*)pl[4].dev;
    hipLaunchKernelGGL(k_moments_read, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, c->stream, c->mom.as<MomRec>(),
                       (uint64_t)npix, D);
    HIPCHK(hipGetLastError());
    if (!on_device)
        for (const Plane& q : pl)
            if (q.host) HIPCHK(hipMemcpyAsync(q.host, q.dev, q.k * npix * 4, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the moments read"));
    return KHP_OK;
}
