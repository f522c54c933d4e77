// denoise_var_dev.h -- khp_denoise_var on the device: the kernels over denoise_var.h's
// per-pixel functions and the entry (included by render.hip after denoise_dev.h).
// Definition: DESIGN.md §17.
//
//   k_dnv_prepare                 a lane per pixel: the planes -> denoise.h's records (n.xyz, d)
//                                 (t.xyz, cv) (c.rgb, fin) and the 8-byte variance record (v, known);
//                                 with KHP_NOISE_CONTEXT the two MomRec of khp_ctx::mom are read in
//                                 place (and the mean as the colour when the caller gave none);
//   k_dnv_atrous<LAST, PREFILTER> once per iteration, k_dn_atrous' 64 x 4 blocks with x fastest on
//                                 a 1-D grid: each of the 25 taps (and of the prefilter's 9) is one
//                                 contiguous row segment per record; the colour and the variance
//                                 records ping-pong together, and the last iteration writes the
//                                 [H][W][3] output and, if asked for, the [H][W] variance instead.
// A pixel's result is a function of the previous iteration's records alone.
//
// Scratch (khp_ctx::dnv, grown on demand, freed with the context): 16 B x (g0, g1, col[0], col[1])
// + 8 B x (var[0], var[1]) = 80 bytes per pixel.
#pragma once

#include "denoise_var.h"

struct DnvScratch {
    DnRec* g0;
    DnRec* g1;
    DnRec* col[2];
    DnVar* var[2];
};

__global__ __launch_bounds__(256) void k_dnv_prepare(DnParams P, DnPlanes G, DnvNoise Z, DnvScratch S, uint64_t npix) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    DnRec g0, g1, col;
    DnVar var;
    dnv_prepare(P, G, Z, (size_t)p, g0, g1, col, var);
    if (P.on & (DN_NORMAL | DN_DEPTH)) S.g0[p] = g0;
    if (P.on & (DN_TANGENT | DN_COVERAGE)) S.g1[p] = g1;
    S.col[0][p] = col;
    S.var[0][p] = var;
}

template <bool LAST, bool PREFILTER>
__global__ __launch_bounds__(DN_BX* DN_BY) void k_dnv_atrous(DnParams P, float floor, const DnRec* __restrict__ g0,
                                                                  const DnRec* __restrict__ g1, const DnRec* __restrict__ cin,
                                                                  const DnVar* __restrict__ vin, DnRec* __restrict__ cout,
                                                                  DnVar* __restrict__ vout, int step, uint32_t blocks_x,
                                                                  float* __restrict__ out, float* __restrict__ out_variance) {
    // a 1-D grid of 2-D blocks, as k_dn_atrous
    const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const uint32_t x = bx * DN_BX + threadIdx.x, y = by * DN_BY + threadIdx.y;
    if (x >= P.W || y >= P.H) return;
    DnVar rv;
    const DnRec r = dnv_filter<PREFILTER>(P, floor, (int)x, (int)y, step, g0, g1, cin, vin, rv);
    const size_t p = (size_t)y * P.W + x;
    if (LAST) {
        out[3 * p] = r.x;
        out[3 * p + 1] = r.y;
        out[3 * p + 2] = r.z;
        if (out_variance) out_variance[p] = dnv_finish_variance(rv);
    } else {
        cout[p] = r;
        vout[p] = rv;
    }
}

// ---- host side ---------------------------------------------------------------------------
struct DnvState {
    DevMem rec;     // the records: 80 bytes per pixel (above)
    DevMem stage;   // host callers: the planes in, the frame and the variance out
};

template <bool PREFILTER>
static void dnv_launch_iterations(khp_ctx* c, const DnParams& P, float floor, const DnvScratch& S, uint32_t iterations,
                                  float* d_out, float* d_outv) {
    const uint32_t blocks_x = (uint32_t)(((uint64_t)P.W + DN_BX - 1) / DN_BX), blocks_y = (uint32_t)(((uint64_t)P.H + DN_BY - 1) / DN_BY);
    const dim3 grid(blocks_x * blocks_y), block(DN_BX, DN_BY);   // < 2^31 blocks: width * height <= 2^31
    for (uint32_t it = 0; it < iterations; ++it) {
        const int src = (int)(it & 1u);
        if (it + 1 < iterations)
            hipLaunchKernelGGL((k_dnv_atrous<false, PREFILTER>), grid, block, 0, c->stream, P, floor, S.g0, S.g1, S.col[src],
                               S.var[src], S.col[src ^ 1], S.var[src ^ 1], 1 << it, blocks_x, d_out, d_outv);
        else
            hipLaunchKernelGGL((k_dnv_atrous<true, PREFILTER>), grid, block, 0, c->stream, P, floor, S.g0, S.g1, S.col[src],
                               S.var[src], S.col[src ^ 1], S.var[src ^ 1], 1 << it, blocks_x, d_out, d_outv);
    }
}

extern "C" khp_status khp_denoise_var(khp_ctx* c, const khp_denoise_params* p, const float* colour,
                                      const khp_aov_buffers* guides, const khp_denoise_noise* noise, float* out) {
    // the arguments first, then the context: every refusal of an argument needs no device
    DnParams P{};
    DnPlanes G{};
    DnvNoise Z{};
    khp_status st;
    if (const char* why = dnv_check(p, colour, guides, noise, out, false, P, G, Z, st)) return fail(st, why);
    if (!c) return fail(KHP_EINVAL, "ctx is null");
    const bool from_ctx = Z.source == KHP_NOISE_CONTEXT;
    if (!colour || from_ctx) {   // state of the context is read: what khp_read_framebuffer does first, and no more
        KHPCHK(drain(c));
        if (from_ctx && !c->moments_on)
            return fail(KHP_ENOTREADY, "KHP_NOISE_CONTEXT: moments are off (khp_set_moments first)");
        if (!c->fb.p || (from_ctx && !c->mom.p))
            return fail(KHP_ENOTREADY, from_ctx ? "KHP_NOISE_CONTEXT: nothing rendered yet"
                                                : "nothing rendered yet: colour is null and there is no framebuffer");
        if (c->fbW != p->width || c->fbH != p->height)
            return fail(KHP_EINVAL, from_ctx ? "KHP_NOISE_CONTEXT: width and height must be the framebuffer's"
                                             : "colour is null: width and height must be the framebuffer's");
    }
    HIPCHK(hipSetDevice(c->device));
    const bool on_device = (p->flags & KHP_DENOISE_DEVICE) != 0;
    const size_t npix = (size_t)P.W * P.H;
    // the planes the call reads, with their 4-byte words per pixel
    const bool cov = dn_reads_coverage(P.on);
    const float* count_words = reinterpret_cast<const float*>(Z.count);   // staged as 4-byte words like the rest
    struct In { const float** ptr; size_t k; bool used; };
    In in[8] = {{&G.colour, 3, colour != nullptr},
                {&G.normal, 3, (P.on & DN_NORMAL) != 0},
                {&G.tangent, 3, (P.on & DN_TANGENT) != 0},
                {&G.depth, 1, (P.on & DN_DEPTH) != 0},
                {&G.coverage, 1, cov},
                {&Z.variance, 1, Z.source == KHP_NOISE_PLANE},
                {&Z.m2, 3, Z.source == KHP_NOISE_MOMENTS},
                {&count_words, 1, Z.source == KHP_NOISE_MOMENTS}};
    float* const outv = Z.out_variance;
    if (on_device) {   // a host pointer here would be read or written by a kernel
        for (const In& q : in)
            if (q.used && !is_device_ptr(*q.ptr))
                return fail(KHP_EINVAL, "KHP_DENOISE_DEVICE: colour, a guide plane or a noise plane is not device memory");
        if (!is_device_ptr(out)) return fail(KHP_EINVAL, "KHP_DENOISE_DEVICE: out is not device memory");
        if (outv && !is_device_ptr(outv)) return fail(KHP_EINVAL, "KHP_DENOISE_DEVICE: out_variance is not device memory");
    }
    if (!c->dnv) c->dnv = std::make_shared<DnvState>();
    DnvState& D = *c->dnv;
    if (D.rec.ensure(npix * (4 * sizeof(DnRec) + 2 * sizeof(DnVar))) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KHP_ENOMEM, "khp_denoise_var: no device memory for 80 bytes per pixel");
    }
    DnvScratch S;
    S.g0 = D.rec.as<DnRec>();
    S.g1 = S.g0 + npix;
    S.col[0] = S.g1 + npix;
    S.col[1] = S.col[0] + npix;
    S.var[0] = (DnVar*)(S.col[1] + npix);
    S.var[1] = S.var[0] + npix;
    float* d_out = out;
    float* d_outv = outv;
    if (!on_device) {   // host buffers go through the staging area
        size_t words = (outv ? 4 : 3) * npix;   // the frame and the variance out
        for (const In& q : in)
            if (q.used) words += q.k * npix;
        HIPCHK(D.stage.ensure(words * 4));
        float* at = D.stage.as<float>();
        d_out = at;
        at += 3 * npix;
        if (outv) {
            d_outv = at;
            at += npix;
        }
        for (In& q : in) {
            if (!q.used) continue;
            HIPCHK(hipMemcpyAsync(at, *q.ptr, q.k * npix * 4, hipMemcpyHostToDevice, c->stream));
            *q.ptr = at;
            at += q.k * npix;
        }
        Z.count = reinterpret_cast<const uint32_t*>(count_words);
    }
    if (from_ctx) {   // read only, in place
        Z.mom = c->mom.as<MomRec>();
        if (!colour) Z.mean = Z.mom;
    } else if (!colour) {
        G.colour = c->fb.as<float>();
    }
    Z.out_variance = nullptr;   // the iterations write it, not the prepare kernel
    hipLaunchKernelGGL(k_dnv_prepare, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, c->stream, P, G, Z, S, (uint64_t)npix);
    if (Z.prefilter) dnv_launch_iterations<true>(c, P, Z.floor, S, p->iterations, d_out, d_outv);
    else dnv_launch_iterations<false>(c, P, Z.floor, S, p->iterations, d_out, d_outv);
    HIPCHK(hipGetLastError());
    if (!on_device) {
        HIPCHK(hipMemcpyAsync(out, d_out, 3 * npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (outv) HIPCHK(hipMemcpyAsync(outv, d_outv, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    KHPCHK(wait_stream(c, c->stream, "the variance-guided denoised frame"));
    return KHP_OK;
}
