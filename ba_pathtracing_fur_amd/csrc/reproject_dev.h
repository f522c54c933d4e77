// reproject_dev.h -- khp_reproject on the device: the kernel over reproject.h's per-pixel
// function and the entry (included by render.hip last, so that every kernel above keeps
// its place in the code object).  Definition: DESIGN.md §18.
//
//   k_reproject   a lane per pixel in k_dn_atrous' 64 x 4 blocks with x fastest on a 1-D
//                 grid: a wave is 64 consecutive pixels of one row.  A camera move maps a row
//                 segment to a (nearly) straight segment of the history, so the four taps of
//                 neighbouring lanes are neighbouring history pixels: every plane's gather is
//                 a few contiguous runs per wave, served by L2.  The history is read plane by
//                 plane, in place: there is no prepare pass and no record scratch.  The four
//                 taps' loads are issued before the first is used.
// A pixel's outputs are a function of the two frames alone: no atomics, no dependence on
// which lane or block computes it.
//
// Like khp_denoise the call is only queued on the context's stream and has its own staging
// area for host callers (khp_ctx::rp, grown on demand, freed with the context).
#pragma once

#include "reproject.h"

__global__ __launch_bounds__(DN_BX* DN_BY) void k_reproject(RpParams P, RpFrame C, RpFrame Hs, RpOut O, uint32_t blocks_x) {
    // a 1-D grid of 2-D blocks, as k_dn_atrous
    const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const uint32_t x = bx * DN_BX + threadIdx.x, y = by * DN_BY + threadIdx.y;
    if (x >= P.W || y >= P.H) return;
    rp_pixel(P, C, Hs, O, x, y);
}

// ---- host side ---------------------------------------------------------------------------
struct RpState {
    DevMem stage;   // host callers: the two frames' planes in, the outputs back
};

extern "C" khp_status khp_reproject(khp_ctx* c, const khp_reproject_params* p, const khp_reproject_frame* cur,
                                    const khp_reproject_frame* hist, const khp_reproject_out* out) {
    // the arguments first, then the context: every refusal of an argument needs no device
    RpParams P{};
    RpFrame C{}, Hs{};
    RpOut O{};
    if (const char* why = rp_check(p, cur, hist, out, false, P, C, Hs, O)) return fail(KHP_EINVAL, why);
    if (!c) return fail(KHP_EINVAL, "ctx is null");
    HIPCHK(hipSetDevice(c->device));
    const bool on_device = (p->flags & KHP_REPROJECT_DEVICE) != 0;
    const size_t npix = (size_t)P.W * P.H;
    // the planes the call reads (rp_check left the others null), with their 4-byte words per pixel
    const float* cur_object = reinterpret_cast<const float*>(C.object);   // staged as 4-byte words like the rest
    const float* hist_object = reinterpret_cast<const float*>(Hs.object);
    struct In { const float** ptr; size_t k; };
    const In in[15] = {{&C.colour, 3},  {&C.variance, 1},  {&C.normal, 3},  {&C.tangent, 3},  {&C.depth, 1},  {&C.coverage, 1},
                       {&cur_object, 1}, {&Hs.colour, 3},  {&Hs.variance, 1}, {&Hs.length, 1}, {&Hs.normal, 3}, {&Hs.tangent, 3},
                       {&Hs.depth, 1},   {&Hs.coverage, 1}, {&hist_object, 1}};
    struct Out { float** ptr; size_t k; float* host; };
    Out outs[4] = {{&O.colour, 3, O.colour}, {&O.length, 1, O.length}, {&O.variance, 1, O.variance}, {&O.motion, 2, O.motion}};
    if (on_device) {   // a host pointer here would be read or written by the kernel
        for (const In& q : in)
            if (*q.ptr && !is_device_ptr(*q.ptr))
                return fail(KHP_EINVAL, "KHP_REPROJECT_DEVICE: a plane of the current or the history frame is not device memory");
        for (const Out& q : outs)
            if (*q.ptr && !is_device_ptr(*q.ptr)) return fail(KHP_EINVAL, "KHP_REPROJECT_DEVICE: an output is not device memory");
    } else {           // host buffers go through the staging area
        if (!c->rp) c->rp = std::make_shared<RpState>();
        size_t words = 0;
        for (const In& q : in)
            if (*q.ptr) words += q.k * npix;
        for (const Out& q : outs)
            if (*q.ptr) words += q.k * npix;
        if (c->rp->stage.ensure(words * 4) != hipSuccess) {
            (void)hipGetLastError();
            return fail(KHP_ENOMEM, "khp_reproject: no device memory to stage the two frames");
        }
        float* at = c->rp->stage.as<float>();
        for (Out& q : outs) {
            if (!*q.ptr) continue;
            *q.ptr = at;
            at += q.k * npix;
        }
        for (const In& q : in) {
            if (!*q.ptr) continue;
            HIPCHK(hipMemcpyAsync(at, *q.ptr, q.k * npix * 4, hipMemcpyHostToDevice, c->stream));
            *q.ptr = at;
            at += q.k * npix;
        }
    }
    C.object = reinterpret_cast<const int32_t*>(cur_object);
    Hs.object = reinterpret_cast<const int32_t*>(hist_object);
    const uint32_t blocks_x = (uint32_t)(((uint64_t)P.W + DN_BX - 1) / DN_BX), blocks_y = (uint32_t)(((uint64_t)P.H + DN_BY - 1) / DN_BY);
    const dim3 grid(blocks_x * blocks_y), block(DN_BX, DN_BY);   // < 2^31 blocks: width * height <= 2^31
    hipLaunchKernelGGL(k_reproject, grid, block, 0, c->stream, P, C, Hs, O, blocks_x);
    HIPCHK(hipGetLastError());
    if (!on_device)
        for (const Out& q : outs)
            if (q.host) HIPCHK(hipMemcpyAsync(q.host, *q.ptr, q.k * npix * 4, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the reprojected frame"));
    return KHP_OK;
}
