// denoise_dev.h -- khp_denoise on the device: the kernels over denoise.h's per-pixel
// functions and the entry (included by render.hip after aov.h).  Definition: DESIGN.md §13.
//
//   k_dn_prepare      a lane per pixel: the planes -> three 16-byte records per pixel
//                     (n.xyz, d) (t.xyz, cv) (c.rgb, fin), and (m.rgb, 0) when demodulating;
//   k_dn_atrous<LAST> once per iteration, 64 x 4 blocks with x fastest: a wave is 64
//                     consecutive pixels of one row, so each of the 25 taps is one
//                     contiguous 1-KiB row segment per record at any step; the colour
//                     records ping-pong between two buffers, and the last iteration
//                     ends in dn_finish and writes the [H][W][3] output instead.
// A pixel's result is a function of the previous iteration's records alone: no
// atomics, no dependence on which lane or block computes it.
//
// Like khp_render_aov the call has its own scratch (khp_ctx::dn, grown on demand,
// freed with the context) and is only queued on the context's stream.
#pragma once

#include "denoise.h"

constexpr int DN_BX = 64, DN_BY = 4;

struct DnScratch {
    DnRec* g0;
    DnRec* g1;
    DnRec* mod;
    DnRec* col[2];
};

__global__ __launch_bounds__(256) void k_dn_prepare(DnParams P, DnPlanes G, DnScratch S, uint64_t npix) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    DnRec g0, g1, col, mod;
    dn_prepare(P, G, (size_t)p, g0, g1, col, mod);
    if (P.on & (DN_NORMAL | DN_DEPTH)) S.g0[p] = g0;
    if (P.on & (DN_TANGENT | DN_COVERAGE)) S.g1[p] = g1;
    if (P.on & DN_DEMOD) S.mod[p] = mod;
    S.col[0][p] = col;
}

template <bool LAST>
__global__ __launch_bounds__(DN_BX* DN_BY) void k_dn_atrous(DnParams P, const DnRec* __restrict__ g0, const DnRec* __restrict__ g1,
                                                                 const DnRec* __restrict__ mods, const DnRec* __restrict__ cin,
                                                                 DnRec* __restrict__ cout, int step, uint32_t blocks_x,
                                                                 float* __restrict__ out) {
    // a 1-D grid of 2-D blocks (a grid's y extent stops at 65535, a frame's height does not)
    const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const uint32_t x = bx * DN_BX + threadIdx.x, y = by * DN_BY + threadIdx.y;
    if (x >= P.W || y >= P.H) return;
    const DnRec r = dn_filter(P, (int)x, (int)y, step, g0, g1, cin);
    const size_t p = (size_t)y * P.W + x;
    if (LAST) {
        DnRec mod = {1.0f, 1.0f, 1.0f, 0.0f};
        if (P.on & DN_DEMOD) mod = mods[p];
        dn_finish(P, r, mod, out + 3 * p);
    } else {
        cout[p] = r;
    }
}

// ---- host side ---------------------------------------------------------------------------
struct DnState {
    DevMem rec;     // the records: 16 B x (g0, g1, mod, col[0], col[1]) per pixel
    DevMem stage;   // host callers: the planes in, the frame out
};

extern "C" khp_status khp_denoise(khp_ctx* c, const khp_denoise_params* p, const float* colour,
                                  const khp_aov_buffers* guides, float* out) {
    // the arguments first, then the context: every refusal of an argument needs no device
    DnParams P{};
    DnPlanes G{};
    if (const char* why = dn_check(p, colour, guides, out, false, P, G)) return fail(KHP_EINVAL, why);
    if (!c) return fail(KHP_EINVAL, "ctx is null");
    if (!colour) {   // the context's framebuffer: what khp_read_framebuffer does first, and no more
        KHPCHK(drain(c));
        if (!c->fb.p) return fail(KHP_ENOTREADY, "nothing rendered yet: colour is null and there is no framebuffer");
        if (c->fbW != p->width || c->fbH != p->height)
            return fail(KHP_EINVAL, "colour is null: width and height must be the framebuffer's");
    }
    HIPCHK(hipSetDevice(c->device));
    const bool on_device = (p->flags & KHP_DENOISE_DEVICE) != 0;
    const size_t npix = (size_t)P.W * P.H;
    // the planes the call reads, in DnPlanes order, with their floats per pixel
    const bool cov = dn_reads_coverage(P.on);
    struct In { const float** ptr; size_t k; bool used; };
    In in[6] = {{&G.colour, 3, colour != nullptr},          {&G.normal, 3, (P.on & DN_NORMAL) != 0},
                {&G.albedo, 3, (P.on & DN_DEMOD) != 0},     {&G.tangent, 3, (P.on & DN_TANGENT) != 0},
                {&G.depth, 1, (P.on & DN_DEPTH) != 0},      {&G.coverage, 1, cov}};
    if (on_device) {   // a host pointer here would be read or written by a kernel
        for (const In& q : in)
            if (q.used && !is_device_ptr(*q.ptr))
                return fail(KHP_EINVAL, "KHP_DENOISE_DEVICE: colour or a guide plane is not device memory");
        if (!is_device_ptr(out)) return fail(KHP_EINVAL, "KHP_DENOISE_DEVICE: out is not device memory");
    }
    if (!c->dn) c->dn = std::make_shared<DnState>();
    DnState& D = *c->dn;
    if (D.rec.ensure(5 * npix * sizeof(DnRec)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KHP_ENOMEM, "khp_denoise: no device memory for 80 bytes per pixel");
    }
    DnScratch S;
    S.g0 = D.rec.as<DnRec>();
    S.g1 = S.g0 + npix;
    S.mod = S.g1 + npix;
    S.col[0] = S.mod + npix;
    S.col[1] = S.col[0] + npix;
    float* d_out = out;
    if (!on_device) {   // host buffers go through the staging area
        size_t floats = 3 * npix;   // the frame out
        for (const In& q : in)
            if (q.used) floats += q.k * npix;
        HIPCHK(D.stage.ensure(floats * sizeof(float)));
        float* at = D.stage.as<float>();
        d_out = at;
        at += 3 * npix;
        for (In& q : in) {
            if (!q.used) continue;
            HIPCHK(hipMemcpyAsync(at, *q.ptr, q.k * npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
            *q.ptr = at;
            at += q.k * npix;
        }
    }
    if (!colour) G.colour = c->fb.as<float>();   // read only
    hipLaunchKernelGGL(k_dn_prepare, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, c->stream, P, G, S, (uint64_t)npix);
    const uint32_t blocks_x = (uint32_t)(((uint64_t)P.W + DN_BX - 1) / DN_BX), blocks_y = (uint32_t)(((uint64_t)P.H + DN_BY - 1) / DN_BY);
    const dim3 grid(blocks_x * blocks_y), block(DN_BX, DN_BY);   // < 2^31 blocks: width * height <= 2^31
    for (uint32_t it = 0; it < p->iterations; ++it) {
        const int src = (int)(it & 1u);
        if (it + 1 < p->iterations) hipLaunchKernelGGL(k_dn_atrous<false>, grid, block, 0, c->stream, P, S.g0, S.g1, S.mod, S.col[src], S.col[src ^ 1],
                                                        1 << it, blocks_x, d_out);
        else hipLaunchKernelGGL(k_dn_atrous<true>, grid, block, 0, c->stream, P, S.g0, S.g1, S.mod, S.col[src], S.col[src ^ 1],
                                                        1 << it, blocks_x, d_out);
    }
    HIPCHK(hipGetLastError());
    if (!on_device) HIPCHK(hipMemcpyAsync(out, d_out, 3 * npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the denoised frame"));
    return KHP_OK;
}
