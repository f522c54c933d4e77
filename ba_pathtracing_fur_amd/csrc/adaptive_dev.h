// adaptive_dev.h -- adaptive passes on the device: the selection kernels, the fold, and the
// entries (included last by render.hip, after moments_dev.h, so that every other kernel keeps
// its place in the code object).  Definition: adaptive.h and DESIGN.md §15.
//
// khp_render_adaptive is a synchronous single pass of the staged batch driver (render.hip:
// plan_batch, reserve_batch, enqueue_chunk, enqueue_bounce) over the ACTIVE pixels instead of
// the owned ones: enqueue_frames asks adaptive_list below for the batch's pixel view, and
// enqueue_accumulate launches k_accumulate_a in place of the running-mean kernels: the same
// body (render.hip's accumulate_frame) compiled with the moments fold and without the mean.
//
// The active list is the owned list with the inactive pixels removed, order kept, made by
// three launches on the context stream -- no atomics, no block waiting on another:
//   k_adapt_flag     a lane per owned pixel: the two records, the rule (adapt_active), one
//                    64-bit ballot per wave stored as the wave's mask word, a count per block;
//   k_adapt_scan     one block: the exclusive scan of the block counts, and the total;
//   k_adapt_scatter  re-reads the mask words: out[block base + earlier waves' popcounts +
//                    popcount(mask & lanes below)] = pixel.
// The total comes back through a pinned word: the pass's one extra synchronisation, since the
// host plans chunks and grids from the count.
#pragma once

#include "adaptive.h"

constexpr uint32_t ADAPT_BLOCK = 256;                 // pixels (lanes) per block of flag and scatter
constexpr uint32_t ADAPT_WAVES = ADAPT_BLOCK / 64;    // mask words per block
constexpr uint32_t ADAPT_SCAN = 1024;                 // block counts k_adapt_scan takes per turn of its loop

__global__ __launch_bounds__(ADAPT_BLOCK) void k_adapt_flag(khp_adaptive_params prm, uint32_t first_sample,
                                                           const MomRec* __restrict__ st,
                                                           const uint32_t* __restrict__ owned, uint32_t n,
                                                           unsigned long long* __restrict__ mask,
                                                           uint32_t* __restrict__ counts) {
    __shared__ uint32_t wcnt[ADAPT_WAVES];
    const uint32_t i = blockIdx.x * ADAPT_BLOCK + threadIdx.x;
    bool act = false;
    if (i < n) {
        const uint32_t pixel = owned[i];
        const MomRec a = st[2 * (size_t)pixel], b = st[2 * (size_t)pixel + 1];
        act = adapt_active(prm, first_sample, a, b);
    }
    const unsigned long long m = __ballot(act);
    const uint32_t w = threadIdx.x >> 6;
    if (lane_id() == 0) {
        mask[(size_t)blockIdx.x * ADAPT_WAVES + w] = m;
        wcnt[w] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < ADAPT_WAVES; ++k) sum += wcnt[k];
        counts[blockIdx.x] = sum;
    }
}

// base[b] = active pixels in the blocks before b; *total = all of them.  One block; more than
// ADAPT_SCAN counts take further turns of the loop, the running total carried along.
__global__ __launch_bounds__(ADAPT_SCAN) void k_adapt_scan(const uint32_t* __restrict__ counts, uint32_t nb,
                                                          uint32_t* __restrict__ base, unsigned long long* total) {
    __shared__ uint32_t part[ADAPT_SCAN];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t t0 = 0; t0 < nb; t0 += ADAPT_SCAN) {
        const uint32_t idx = t0 + t;
        const uint32_t own = idx < nb ? counts[idx] : 0u;
        part[t] = own;
        __syncthreads();
        for (uint32_t off = 1; off < ADAPT_SCAN; off <<= 1) {   // inclusive Hillis-Steele scan
            const uint32_t v = t >= off ? part[t - off] : 0u;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        if (idx < nb) base[idx] = carry + part[t] - own;
        carry += part[ADAPT_SCAN - 1];
        __syncthreads();   // every thread has read the turn's total before the next turn overwrites it
    }
    if (t == 0) *total = carry;
}

__global__ __launch_bounds__(ADAPT_BLOCK) void k_adapt_scatter(const uint32_t* __restrict__ owned, uint32_t n,
                                                              const unsigned long long* __restrict__ mask,
                                                              const uint32_t* __restrict__ base,
                                                              uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * ADAPT_BLOCK + threadIdx.x;
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    const unsigned long long* bm = mask + (size_t)blockIdx.x * ADAPT_WAVES;
    uint32_t at = base[blockIdx.x];
    for (uint32_t k = 0; k < w; ++k) at += (uint32_t)__popcll(bm[k]);
    const unsigned long long m = bm[w];
    if (i < n && ((m >> lane) & 1ull)) out[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = owned[i];
}

// The fold of an adaptive batch: k_accumulate_m's body (render.hip: accumulate_frame) without the
// running mean.  A lane per active pixel, its two records loaded once and stored once, the chunk's
// samples folded in increasing k, and the framebuffer pixel stored from the mean.  One frame
// (nf == 1): a pixel's samples are adjacent 16-byte paths under either path numbering.
__global__ __launch_bounds__(256) void k_accumulate_a(Wave Wv, float* fb, uint32_t fr, MomRec* st) {
    accumulate_frame<false, true>(Wv, fb, fr, st);
}

// ---- host side ---------------------------------------------------------------------------
// What one selection needs beside its inputs; `list` receives the active pixels.
struct AdaptScratch {
    DevMem mask, counts, base, total, list;
    unsigned long long* htotal = nullptr;   // pinned: the count the host plans from
    hipEvent_t e0 = nullptr, e1 = nullptr;  // around the launches and the count's copy
    double ms = 0.0;                        // the last selection between them
    ~AdaptScratch() {
        if (htotal) (void)hipHostFree(htotal);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};
struct AdaptState {
    AdaptScratch pass;              // khp_render_adaptive's; pass.list holds the last pass's n_last pixels
    uint32_t n_last = 0;
    bool have_last = false;
    AdaptScratch dbg;               // khp_debug_adaptive_select's own
    DevMem dbg_state, dbg_owned;
};

// The three launches on s and the count's readback; returns once the count is known.
static khp_status adapt_select(khp_ctx* c, AdaptScratch& A, hipStream_t s, const khp_adaptive_params& prm,
                               uint32_t first_sample, const MomRec* st, const uint32_t* owned, uint32_t n_owned,
                               uint32_t* n_active) {
    *n_active = 0;
    if (n_owned == 0) return KHP_OK;
    const uint32_t nb = (n_owned + ADAPT_BLOCK - 1) / ADAPT_BLOCK;
    if (A.mask.ensure((size_t)nb * ADAPT_WAVES * sizeof(unsigned long long)) != hipSuccess ||
        A.counts.ensure((size_t)nb * sizeof(uint32_t)) != hipSuccess ||
        A.base.ensure((size_t)nb * sizeof(uint32_t)) != hipSuccess ||
        A.total.ensure(sizeof(unsigned long long)) != hipSuccess ||
        A.list.ensure((size_t)n_owned * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KHP_ENOMEM, "khp_render_adaptive: no device memory for the pixel selection");
    }
    if (!A.htotal) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&A.htotal), sizeof(unsigned long long), hipHostMallocDefault));
    if (!A.e0) HIPCHK(hipEventCreate(&A.e0));
    if (!A.e1) HIPCHK(hipEventCreate(&A.e1));
    HIPCHK(hipEventRecord(A.e0, s));
    hipLaunchKernelGGL(k_adapt_flag, dim3(nb), dim3(ADAPT_BLOCK), 0, s, prm, first_sample, st, owned, n_owned,
                       A.mask.as<unsigned long long>(), A.counts.as<uint32_t>());
    hipLaunchKernelGGL(k_adapt_scan, dim3(1), dim3(ADAPT_SCAN), 0, s, A.counts.as<uint32_t>(), nb, A.base.as<uint32_t>(),
                       A.total.as<unsigned long long>());
    hipLaunchKernelGGL(k_adapt_scatter, dim3(nb), dim3(ADAPT_BLOCK), 0, s, owned, n_owned,
                       A.mask.as<unsigned long long>(), A.base.as<uint32_t>(), A.list.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(A.htotal, A.total.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(A.e1, s));
    KHPCHK(wait_stream(c, s, "the pixel selection"));
    float ms = 0.0f;
    A.ms = hipEventElapsedTime(&ms, A.e0, A.e1) == hipSuccess ? (double)ms : 0.0;
    if (*A.htotal > n_owned) return fail(KHP_EDEVICE, "internal: the pixel selection counted more pixels than are owned");
    *n_active = (uint32_t)*A.htotal;
    return KHP_OK;
}

// enqueue_frames' pixel view of an adaptive batch: the active pixels among the owned ones (c->pix, made by
// open_batch just before), chosen from the state as it stands on the context stream.
static khp_status adaptive_list(khp_ctx* c, const khp_render_params* p, const AdaptPass& ad, const uint32_t** pix,
                                uint32_t* n) {
    if (!c->ad) c->ad = std::make_shared<AdaptState>();
    AdaptState& A = *c->ad;
    const uint32_t n_owned = (uint32_t)c->pix_host.size();
    A.have_last = false;
    uint32_t n_active = 0;
    if (c->fb_evt) HIPCHK(hipStreamWaitEvent(c->stream, c->fb_evt, 0));   // the state's last writer
    KHPCHK(adapt_select(c, A.pass, c->stream, *ad.prm, p->first_sample, c->mom.as<MomRec>(), c->pix.as<uint32_t>(),
                        n_owned, &n_active));
    A.n_last = n_active;
    A.have_last = true;
    if (ad.res) {
        *ad.res = khp_adaptive_result{};
        ad.res->owned = n_owned;
        ad.res->active = n_active;
    }
    *pix = A.pass.list.as<uint32_t>();
    *n = n_active;
    return KHP_OK;
}

extern "C" khp_status khp_render_adaptive(khp_ctx* c, const khp_render_params* p, const khp_adaptive_params* a,
                                          khp_adaptive_result* res, float* out_rgb) {
    // the arguments first, then the context: every refusal leaves state and framebuffer as they are
    if (!c || !p || !a) return fail(KHP_EINVAL, "khp_render_adaptive: null argument");
    if (const char* why = adapt_params_error(a)) return fail(KHP_EINVAL, std::string("khp_render_adaptive: ") + why);
    if (p->spp == 0 || p->spp > (1u << 24)) return fail(KHP_EINVAL, "khp_render_adaptive: spp must be 1 .. 2^24");
    if (p->flags & ~(uint32_t)(KHP_RENDER_OUT_DEVICE | KHP_RENDER_NO_READBACK))
        return fail(KHP_EINVAL, "khp_render_adaptive: flags may be KHP_RENDER_OUT_DEVICE or KHP_RENDER_NO_READBACK "
                                "(no KHP_RENDER_ASYNC, no KHP_RENDER_STATS)");
    if ((uint64_t)p->first_sample + p->spp > 0xFFFFFFFFull)
        return fail(KHP_EINVAL, "khp_render_adaptive: first_sample + spp overflows");
    KHPCHK(check_params(c, p));
    if (!c->moments_on) return fail(KHP_ENOTREADY, "khp_render_adaptive: moments are off (khp_set_moments first)");
    if (light_paths_on(c))
        return fail(KHP_EUNSUPPORTED, "khp_render_adaptive: not with the light-path variant (khp_set_bdpt) enabled");
    HIPCHK(hipSetDevice(c->device));
    KHPCHK(flush(c));
    // nothing rendered ahead for another call serves this one, or is served by it
    c->ra.next.valid = false;
    c->wa.next.valid = false;
    c->series.valid = false;
    const AdaptPass ad{a, res};
    return enqueue_frames(c, p, out_rgb, nullptr, &ad);
}

extern "C" khp_status khp_debug_adaptive_list(khp_ctx* c, uint32_t* n, uint32_t* pixels, double* select_ms) {
    if (!c || !n) return fail(KHP_EINVAL, "null argument");
    if (!c->ad || !c->ad->have_last) return fail(KHP_ENOTREADY, "khp_debug_adaptive_list: no adaptive pass yet");
    HIPCHK(hipSetDevice(c->device));
    *n = c->ad->n_last;
    if (select_ms) *select_ms = c->ad->pass.ms;
    if (pixels && *n) HIPCHK(hipMemcpy(pixels, c->ad->pass.list.p, (size_t)*n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return KHP_OK;
}

extern "C" khp_status khp_debug_adaptive_select(khp_ctx* c, const khp_adaptive_params* a, uint32_t first_sample,
                                                uint32_t n_pixels, const khp_moments_buffers* state, uint32_t n_owned,
                                                const uint32_t* owned, uint32_t* active, uint32_t* n_active) {
    if (!c || !a || !state || !n_active) return fail(KHP_EINVAL, "khp_debug_adaptive_select: null argument");
    if (const char* why = adapt_params_error(a)) return fail(KHP_EINVAL, std::string("khp_debug_adaptive_select: ") + why);
    if (!state->mean || !state->m2 || !state->count || !state->bad)
        return fail(KHP_EINVAL, "khp_debug_adaptive_select: a null state plane (mean, m2, count and bad are needed)");
    if (n_owned != 0u && (!owned || !active)) return fail(KHP_EINVAL, "khp_debug_adaptive_select: null pixel list");
    for (uint32_t i = 0; i < n_owned; ++i)   // the kernels index the state by these
        if (owned[i] >= n_pixels)
            return fail(KHP_EINVAL, "khp_debug_adaptive_select: owned[" + std::to_string(i) + "] is not below n_pixels");
    *n_active = 0;
    if (n_owned == 0) return KHP_OK;
    HIPCHK(hipSetDevice(c->device));
    if (!c->ad) c->ad = std::make_shared<AdaptState>();
    AdaptState& A = *c->ad;
    std::vector<MomRec> rec(2 * (size_t)n_pixels);
    for (size_t q = 0; q < n_pixels; ++q) {
        rec[2 * q] = MomRec{state->mean[3 * q], state->mean[3 * q + 1], state->mean[3 * q + 2], state->count[q]};
        rec[2 * q + 1] = MomRec{state->m2[3 * q], state->m2[3 * q + 1], state->m2[3 * q + 2], state->bad[q]};
    }
    if (upload(A.dbg_state, rec.data(), rec.size(), c->stream) != hipSuccess ||
        upload(A.dbg_owned, owned, (size_t)n_owned, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KHP_ENOMEM, "khp_debug_adaptive_select: no device memory for the state and the list");
    }
    uint32_t na = 0;
    KHPCHK(adapt_select(c, A.dbg, c->stream, *a, first_sample, A.dbg_state.as<MomRec>(), A.dbg_owned.as<uint32_t>(),
                        n_owned, &na));
    if (na) HIPCHK(hipMemcpy(active, A.dbg.list.p, (size_t)na * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *n_active = na;
    return KHP_OK;
}
