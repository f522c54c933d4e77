// aov.h -- khp_render_aov: the first hit's features per pixel (normal, albedo,
// fibre tangent, depth, coverage, object id), the buffers a denoiser or a
// compositor wants beside the colour (included by render.hip after
// debug_query.h).  KIRK has no counterpart.  Definition: DESIGN.md §12.
//
// Two kernels per chunk of pixels:
//   k_aov_trace<TEX>: k_extend's camera-bounce loop (persistent grid, lane refill,
//     LDS stack rings, the 64-B records in trace_closest's visit order); a lane owns
//     one sample, computes its camera ray in place (camera_path), and when its
//     traversal ends makes the renderer's light test (k_shade's loop), calls
//     surface_at<TEX> and writes one record, SoA by channel, only the channels
//     asked for;
//   k_aov_reduce: a lane per pixel sums its spp records in sample order (float32
//     adds from +0), divides by (float)spp and writes the planar outputs.
// No float atomics and no order that depends on scheduling: which lane traces
// which sample changes no record, and the sum's order is the sample order.
//
// The call reads the scene, the tree and the camera and writes only its own
// scratch (khp_ctx::aov) and the caller's buffers: no framebuffer, sample
// counter, statistic, path set, pixel list or generation of the context changes,
// and nothing is drained -- asynchronous frames pending or in flight and parked
// render-ahead work stay as they are; the call is only queued behind whatever
// the context stream holds.
#pragma once

// Measured at the metric row: 6 waves per SIMD (80 VGPRs, 76 B of scratch
// per lane in the record path) against 5 (96, none): the same; 8 (64 VGPRs, 140 B): 1.16x
// the time; the record function out of line at 6 / 8 waves (624 / 688 B): 1.55x / 2.2x.
#ifndef KHP_AOV_RING
#define KHP_AOV_RING 6
#endif
#ifndef KHP_AOV_WAVES
#define KHP_AOV_WAVES 6
#endif
#ifndef KHP_AOV_REFILL
#define KHP_AOV_REFILL KHP_REFILL_CAM
#endif
constexpr int AOV_RING = KHP_AOV_RING;
constexpr int AOV_WAVES = KHP_AOV_WAVES;
constexpr size_t AOV_LDS_BYTES = 3 * AOV_RING * TRAV_BLOCK * sizeof(uint32_t);
constexpr uint32_t AOV_MAX_SPP = 1u << 24;   // a pixel's records stay in one chunk

// Per-sample records of a chunk, SoA by channel: column[path], path = chunk pixel
// x spp + sample; obj is per chunk pixel (sample first_sample only).  Null: the
// channel was not asked for and is neither computed into memory nor summed.
struct AovCols {
    float* nrm[3];
    float* alb[3];
    float* tan[3];
    float* depth;
    float* cov;
    int32_t* obj;
};

// The planar outputs ([H][W][3] / [H][W], indexed by the image pixel).
struct AovOut {
    float* normal;
    float* albedo;
    float* tangent;
    float* depth;
    float* coverage;
    int32_t* object;
};

// The record of path idx, whose traversal ended with hit h (slot -1: none).
template <bool TEX>
__device__ __forceinline__ void aov_record(const DevScene& S, const Wave& Wv, const AovCols& R, uint32_t idx,
                                           const Ray& r, const Hit& h) {
    bool surf = h.slot >= 0;
    if (surf) {   // KIRK's linear ray-light test (k_shade; CPU_PathTracer.cpp:185-208): a nearer light ends the path
        float t_lights = FLT_MAX_;
        for (int li = 0; li < S.n_lights; ++li) {
            float t = FLT_MAX_;
            if (light_isect(S.lights[li], r, t)) t_lights = gmin(t_lights, t);
        }
        surf = !(t_lights < h.t);
    }
    v3 n = mk(0.0f, 0.0f, 0.0f), a = n, tg = n;
    float d = 0.0f, cv = 0.0f;
    int32_t ob = -1;
    if (surf) {
        ShadeCtx s;
        khp_material mres;
        const Hit hh{h.t, h.slot, 0.0f, 0.0f};   // u, v: surface_at recomputes them
        n = surface_at<TEX>(S, r, hh, s, mres);
        tg = s.V;
        a = mk(s.m->diffuse[0], s.m->diffuse[1], s.m->diffuse[2]);
        d = h.t;
        cv = 1.0f;
        ob = (int32_t)S.aux[h.slot].obj;
    }
    if (R.nrm[0]) { R.nrm[0][idx] = n.x; R.nrm[1][idx] = n.y; R.nrm[2][idx] = n.z; }
    if (R.alb[0]) { R.alb[0][idx] = a.x; R.alb[1][idx] = a.y; R.alb[2][idx] = a.z; }
    if (R.tan[0]) { R.tan[0][idx] = tg.x; R.tan[1][idx] = tg.y; R.tan[2][idx] = tg.z; }
    if (R.depth) R.depth[idx] = d;
    if (R.cov) R.cov[idx] = cv;
    if (R.obj) {
        const uint32_t p_local = idx / Wv.n_samples;
        if (idx - p_local * Wv.n_samples == 0u) R.obj[p_local] = ob;
    }
}

// k_extend<false, true>'s loop over the chunk's paths (queue slot = path, one
// fused frame), ending each path in aov_record instead of the hit columns.
// LENS: the camera rays are lens rays (khp_set_lens, camera_path<true>).
template <bool TEX, bool LENS = false>
__global__ __launch_bounds__(TRAV_BLOCK, AOV_WAVES) void k_aov_trace(DevScene S, Wave Wv, SpillArea spill, AovCols R) {
    extern __shared__ uint32_t lds[];
    const uint32_t n = Wv.cnt->nq[0];
    LdsStack<AOV_RING, false> stk;
    stk.init(lds, spill.base, spill.stride);
    TravStats st{0, 0, 0};
    TravRay tr;
    Hit h;
    Cur c{0u, 0.0f, 0.0f, false};
    LeafCur lf{0u, 0u, 0.0f, 0.0f, 0.0f, 0.0f, -1};
    bool has = false, exhausted = false;
    uint32_t idx = 0, mode = 0u;
    Claimer cl;
    cl.init(Wv.cnt->fetch_ext, n, 0u, Wv.cap);
    constexpr int refill = KHP_AOV_REFILL;
    for (;;) {
        unsigned long long idle = __ballot(!has);
        if (!exhausted && __popcll(idle) >= refill) {
            uint32_t my;
            const bool got = cl.claim(idle, my, exhausted);
            if (!has && got && cl.phys(my, idx)) {
                uint32_t key_unused;
                const Ray r = camera_path<LENS>(S, Wv, idx, key_unused);
                trav_setup(tr, r);
                h.t = FLT_MAX_;
                h.slot = -1;
                h.u = h.v = 0.0f;
                lf.left = 0;
                has = !ray_has_nan(r) && trav2_begin<false>(S, tr, h.t, stk, mode, c, lf, st);
                if (!has) aov_record<TEX>(S, Wv, R, idx, r, h);   // missed the root box, or a NaN ray (no hit)
            }
        }
        unsigned long long act = __ballot(has);
        if (act == 0) {
            if (exhausted) break;
            continue;
        }
        for (;;) {
            if (has) {
                bool occ_unused;
                if (iter2<false, false>(S, tr, h, 0.0f, stk, mode, c, lf, st, occ_unused)) {
                    aov_record<TEX>(S, Wv, R, idx, tr.r, h);
                    has = false;
                }
            }
            act = __ballot(has);
            if (act == 0 || (!exhausted && 64 - __popcll(act) >= refill)) break;
        }
    }
}

// One lane per chunk pixel: s = +0, s += record k for k = 0 .. spp-1, s / (float)spp.
__device__ __forceinline__ float aov_mean(const float* col, size_t base, uint32_t spp) {
    float s = 0.0f;
    for (uint32_t k = 0; k < spp; ++k) s = s + col[base + k];
    return s / (float)spp;
}
__global__ __launch_bounds__(256) void k_aov_reduce(AovCols R, AovOut O, const uint32_t* __restrict__ pix, uint32_t p_off,
                                                    uint32_t P, uint32_t spp) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const size_t px = pix[p_off + p], base = (size_t)p * spp;
    if (O.normal)
        for (int k = 0; k < 3; ++k) O.normal[3 * px + k] = aov_mean(R.nrm[k], base, spp);
    if (O.albedo)
        for (int k = 0; k < 3; ++k) O.albedo[3 * px + k] = aov_mean(R.alb[k], base, spp);
    if (O.tangent)
        for (int k = 0; k < 3; ++k) O.tangent[3 * px + k] = aov_mean(R.tan[k], base, spp);
    if (O.depth) O.depth[px] = aov_mean(R.depth, base, spp);
    if (O.coverage) O.coverage[px] = aov_mean(R.cov, base, spp);
    if (O.object) O.object[px] = R.obj[p];
}

// ---- host side ---------------------------------------------------------------------------
template <size_t I> struct AovK { static constexpr auto k = k_aov_trace<AOV_TABLE[I].tex, AOV_TABLE[I].lens>; };
// The call's own device state (khp_ctx::aov): nothing of it is shared with the
// renderer, whose path sets, pixel list and spill columns may be in use by
// frames in flight.
struct AovState {
    DevMem rec, obj, cnt, spill, pix, stage;
    std::vector<uint32_t> pix_host;
    TileKey pix_key;
    int grid[2] = {0, 0};   // k_aov_trace<false> / <true>: resident blocks
    std::vector<float> host_tmp;
};

static khp_status aov_pixels(khp_ctx* c, AovState& A, const khp_render_params* p) {
    const TileKey key = tile_key(*p);
    if (key == A.pix_key && A.pix.p) return KHP_OK;
    key.pixels(A.pix_host);
    HIPCHK(upload(A.pix, A.pix_host.data(), A.pix_host.size(), c->stream));
    A.pix_key = key;
    return KHP_OK;
}

extern "C" khp_status khp_render_aov(khp_ctx* c, const khp_render_params* p, const khp_aov_buffers* out) {
    // the arguments first, then the context: every refusal of an argument needs no device
    if (!p || !out) return fail(KHP_EINVAL, "null argument");
    if (!out->normal && !out->albedo && !out->tangent && !out->depth && !out->coverage && !out->object)
        return fail(KHP_EINVAL, "every buffer of khp_aov_buffers is null");
    if (p->flags & ~KHP_RENDER_OUT_DEVICE) return fail(KHP_EINVAL, "flags: only KHP_RENDER_OUT_DEVICE applies to khp_render_aov");
    if (p->spp == 0) return fail(KHP_EINVAL, "spp must be > 0");
    if (p->spp > AOV_MAX_SPP) return fail(KHP_EINVAL, "spp must be at most 2^24");
    if ((uint64_t)p->width * p->height == 0) return fail(KHP_EINVAL, "width * height must be > 0");
    if ((uint64_t)p->width * p->height >= (1ull << 31)) return fail(KHP_EINVAL, "image too large");
    if (tile_key(*p).tile % 8 != 0) return fail(KHP_EINVAL, "tile_size must be a multiple of 8");
    if (p->tile_nranks > 1 && p->tile_rank >= p->tile_nranks) return fail(KHP_EINVAL, "tile_rank >= tile_nranks");
    if (!c) return fail(KHP_EINVAL, "ctx is null");
    if (!c->scene_set) return fail(KHP_ENOTREADY, "khp_set_scene first");
    if (!c->built) return fail(KHP_ENOTREADY, "khp_build_accel first");
    HIPCHK(hipSetDevice(c->device));
    const bool to_device = (p->flags & KHP_RENDER_OUT_DEVICE) != 0;
    if (to_device) {   // a host pointer here would be written by a kernel
        const void* ptrs[6] = {out->normal, out->albedo, out->tangent, out->depth, out->coverage, out->object};
        for (const void* q : ptrs)
            if (q && !is_device_ptr(q))
                return fail(KHP_EINVAL, "KHP_RENDER_OUT_DEVICE: a khp_aov_buffers pointer is not device memory");
    }
    if (!c->aov) c->aov = std::make_shared<AovState>();
    AovState& A = *c->aov;
    const AovVariant va = select_aov(variant_facts(c));   // khp_set_lens: the lens twins (the same launch bounds and grid)
    const bool tex = va.tex;
    if (!A.grid[tex])   // sized from the instance without the lens, whichever runs
        KHPCHK(variant_grid<AovK>(c, AOV_TABLE, {tex, false}, TRAV_BLOCK, AOV_LDS_BYTES, A.grid[tex]));
    // chunks of whole pixels under the context's chunk_paths rule (decided before the scratch takes memory)
    const size_t cap_paths = std::max<size_t>(4096, chunk_paths(c));
    KHPCHK(aov_pixels(c, A, p));
    const uint32_t P_all = (uint32_t)A.pix_host.size();
    if (P_all == 0) return KHP_OK;   // this rank owns no tile
    const uint32_t spp = p->spp;
    const uint32_t P_chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(P_all, cap_paths / spp));
    const size_t n_chunk = (size_t)P_chunk * spp;   // < 2^31: P_chunk * spp <= max(cap_paths, spp)
    if (n_chunk >= ((size_t)1 << 31)) return fail(KHP_EINVAL, "chunk_paths: a chunk of 2^31 paths or more");
    const size_t npix = (size_t)p->width * p->height;
    const int grid = A.grid[tex];
    // scratch: the record columns asked for, the object column, claim cursors, stack spill columns
    const size_t n_cols = (out->normal ? 3 : 0) + (out->albedo ? 3 : 0) + (out->tangent ? 3 : 0) + (out->depth ? 1 : 0) +
                          (out->coverage ? 1 : 0);
    HIPCHK(A.rec.ensure(std::max<size_t>(1, n_cols) * n_chunk * sizeof(float)));
    HIPCHK(A.obj.ensure((size_t)P_chunk * sizeof(int32_t)));
    HIPCHK(A.cnt.ensure(sizeof(Counters)));
    HIPCHK(A.spill.ensure((size_t)grid * TRAV_BLOCK * STACK_MAX * sizeof(int4)));
    AovCols R{};
    {
        float* col = A.rec.as<float>();
        auto take = [&]() { float* q = col; col += n_chunk; return q; };
        if (out->normal) for (int k = 0; k < 3; ++k) R.nrm[k] = take();
        if (out->albedo) for (int k = 0; k < 3; ++k) R.alb[k] = take();
        if (out->tangent) for (int k = 0; k < 3; ++k) R.tan[k] = take();
        if (out->depth) R.depth = take();
        if (out->coverage) R.cov = take();
        if (out->object) R.obj = A.obj.as<int32_t>();
    }
    // outputs: the caller's device buffers, or full-frame staging planes copied (owned pixels only) to the host
    AovOut O{out->normal, out->albedo, out->tangent, out->depth, out->coverage, out->object};
    if (!to_device) {
        const size_t planes = (out->normal ? 3 : 0) + (out->albedo ? 3 : 0) + (out->tangent ? 3 : 0) +
                              (out->depth ? 1 : 0) + (out->coverage ? 1 : 0) + (out->object ? 1 : 0);
        HIPCHK(A.stage.ensure(planes * npix * sizeof(float)));
        float* q = A.stage.as<float>();
        auto take = [&](size_t k) { float* r = q; q += k * npix; return r; };
        O.normal = out->normal ? take(3) : nullptr;
        O.albedo = out->albedo ? take(3) : nullptr;
        O.tangent = out->tangent ? take(3) : nullptr;
        O.depth = out->depth ? take(1) : nullptr;
        O.coverage = out->coverage ? take(1) : nullptr;
        O.object = out->object ? reinterpret_cast<int32_t*>(take(1)) : nullptr;
    }
    Wave Wv{};
    Wv.cnt = A.cnt.as<Counters>();
    Wv.pix = A.pix.as<uint32_t>();
    Wv.W = p->width;
    Wv.H = p->height;
    Wv.seed = p->seed;
    Wv.sample0 = p->first_sample;
    Wv.n_samples = spp;
    Wv.n_frames = 1;
    Wv.pix_major = 1;
    Wv.fsample0[0] = p->first_sample;
    const SpillArea sp{A.spill.as<int4>(), (uint32_t)grid * TRAV_BLOCK};
    for (uint32_t p_off = 0; p_off < P_all; p_off += P_chunk) {
        const uint32_t P = std::min(P_chunk, P_all - p_off), n = P * spp;
        Wv.P = P;
        Wv.p_off = p_off;
        Wv.cap = n;
        HIPCHK(hipMemsetAsync(A.cnt.p, 0, sizeof(Counters), c->stream));
        hipLaunchKernelGGL(k_start, dim3(1), dim3(1), 0, c->stream, Wv.cnt, n);
        KHPCHK(launch_variant<AovK>(AOV_TABLE, va, grid, TRAV_BLOCK, AOV_LDS_BYTES, c->stream, c->S, Wv, sp, R));
        hipLaunchKernelGGL(k_aov_reduce, dim3((P + 255) / 256), dim3(256), 0, c->stream, R, O, Wv.pix, p_off, P, spp);
        HIPCHK(hipGetLastError());
    }
    if (to_device) {
        KHPCHK(wait_stream(c, c->stream, "the feature buffers"));
        return KHP_OK;
    }
    struct Plane { void* host; const void* dev; size_t k; };
    const Plane pl[6] = {{out->normal, O.normal, 3}, {out->albedo, O.albedo, 3}, {out->tangent, O.tangent, 3},
                         {out->depth, O.depth, 1}, {out->coverage, O.coverage, 1}, {out->object, O.object, 1}};
    if (P_all == npix) {   // every pixel is this rank's: the planes as they are
        for (const Plane& q : pl)
            if (q.host) HIPCHK(hipMemcpyAsync(q.host, q.dev, q.k * npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        KHPCHK(wait_stream(c, c->stream, "the feature buffers"));
        return KHP_OK;
    }
    // a tile rank: the owned pixels only, the others stay as the caller left them
    for (const Plane& q : pl) {
        if (!q.host) continue;
        A.host_tmp.resize(q.k * npix);
        HIPCHK(hipMemcpyAsync(A.host_tmp.data(), q.dev, q.k * npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        KHPCHK(wait_stream(c, c->stream, "the feature buffers"));
        float* dst = static_cast<float*>(q.host);   // int32 object ids move as 4-byte words
        for (const uint32_t px : A.pix_host)
            memcpy(dst + q.k * (size_t)px, A.host_tmp.data() + q.k * (size_t)px, q.k * sizeof(float));
    }
    return KHP_OK;
}
