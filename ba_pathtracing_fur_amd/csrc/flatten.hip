// flatten.hip -- CPU::Scene::flattenNode's per-object work on the device
// (SURVEY §8(f)2): the Triangle / Cylinder ctor state of every object, and the
// seeded hairball and the fur of a triangle mesh (Mesh::addFurToFaces + the
// fiber -> cone rule of CPU_Scene.cpp:121-144) generated straight into HBM.  The arithmetic is
// objects.h, the same source the host flatten (scene.cpp) runs.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <string>

#include "device_build.h"
#include "kmath_ops.h"
#include "objects.h"

namespace khp {
namespace fl {

// x - x is 0 for a finite x and NaN for an infinity or a NaN: a sum of such terms is 0 only if all are finite
__device__ __forceinline__ bool all_finite(v3 a, v3 b, v3 c) {
    const v3 d = ((a - a) + (b - b)) + (c - c);
    return (d.x + d.y) + d.z == 0.0f;
}

// err bits: 1 triangle material, 2 cone material, 4 cone model, 8 tri_v, 16 cone_base_r0,
// 32 cone_apex_r1 not finite, 64 finite geometry whose box or centroid overflows float32.
// tm / cm null: the geometry part alone (device_reflatten), the aux words' mat / obj / flags kept.
__global__ void k_flatten_tris(const float* __restrict__ tv, const float* __restrict__ tn,
                               const uint32_t* __restrict__ tm, const float* __restrict__ uv_in, uint32_t n_tris,
                               uint32_t n_mat, float4* rec, Aux* aux, float* bounds, float* cen, float* nrm,
                               float* uv_out, uint32_t* err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tris) return;
    const float* v = tv + 9 * (size_t)i;
    const float* n = tn + 9 * (size_t)i;
    float r[16], bnd[6], ce[3];  // box and centroid stay in registers for the overflow check
    tri_object(ld3(v), ld3(v + 3), ld3(v + 6), ld3(n), ld3(n + 3), ld3(n + 6), r, bnd, ce, nrm + 9 * (size_t)i,
               uv_in ? uv_in + 6 * (size_t)i : nullptr, uv_out ? uv_out + 6 * (size_t)i : nullptr);
    for (int q = 0; q < 6; ++q) bounds[6 * (size_t)i + q] = bnd[q];
    for (int q = 0; q < 3; ++q) cen[3 * (size_t)i + q] = ce[q];
    float4* o = rec + 4 * (size_t)i;
    o[0] = make_float4(r[0], r[1], r[2], r[3]);
    o[1] = make_float4(r[4], r[5], r[6], r[7]);
    o[2] = make_float4(r[8], r[9], r[10], r[11]);
    o[3] = make_float4(r[12], r[13], r[14], r[15]);
    if (!all_finite(ld3(v), ld3(v + 3), ld3(v + 6))) atomicOr(err, 8u);
    else if (!all_finite(ld3(bnd), ld3(bnd + 3), ld3(ce))) atomicOr(err, 64u);
    if (!tm) return;  // geometry only (device_reflatten): a triangle's aux word holds none
    const uint32_t m = tm[i];
    if (m >= n_mat) atomicOr(err, 1u);
    aux[i] = Aux{0.0f, m, i, 0u};
}

// models: n_models x (M, inverse transpose) = 25 floats each, or null (world-space cones)
__global__ void k_flatten_cones(const float4* __restrict__ b, const float4* __restrict__ a,
                                const uint32_t* __restrict__ cm, const uint32_t* __restrict__ cmod,
                                const float* __restrict__ models, uint32_t n_models, uint32_t n_cones, uint32_t id0,
                                uint32_t n_mat, float4* rec, Aux* aux, float* bounds, float* cen, float* cone_h,
                                uint32_t* err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cones) return;
    const uint32_t id = id0 + i;
    const float4 bb = b[i], aa = a[i];
    const v3 base = mk(bb.x, bb.y, bb.z), apex = mk(aa.x, aa.y, aa.z);
    float r[16], bnd[6], ce[3];  // box and centroid stay in registers for the overflow check
    float base_d;
    if (models) {
        uint32_t k = cmod ? cmod[i] : 0u;
        if (k >= n_models) {
            atomicOr(err, 4u);
            k = 0;
        }
        const float* M = models + 25 * (size_t)k;
        base_d = cone_object_xf(base, apex, bb.w, aa.w, M, M + 16, r, bnd, ce);
    } else {
        base_d = cone_object(base, apex, bb.w, aa.w, r, bnd, ce);
    }
    for (int q = 0; q < 6; ++q) bounds[6 * (size_t)id + q] = bnd[q];
    for (int q = 0; q < 3; ++q) cen[3 * (size_t)id + q] = ce[q];
    if (cone_h) cone_h[i] = length(apex - base);  // Cylinder::m_height (pre-transform)
    float4* o = rec + 4 * (size_t)id;
    o[0] = make_float4(r[0], r[1], r[2], r[3]);
    o[1] = make_float4(r[4], r[5], r[6], r[7]);
    o[2] = make_float4(r[8], r[9], r[10], r[11]);
    o[3] = make_float4(r[12], r[13], r[14], r[15]);
    const bool base_ok = all_finite(base, mk(bb.w, 0.0f, 0.0f), mk(0.0f, 0.0f, 0.0f));
    const bool apex_ok = all_finite(apex, mk(aa.w, 0.0f, 0.0f), mk(0.0f, 0.0f, 0.0f));
    if (!base_ok) atomicOr(err, 16u);
    if (!apex_ok) atomicOr(err, 32u);
    if (base_ok && apex_ok && !all_finite(ld3(bnd), ld3(bnd + 3), ld3(ce))) atomicOr(err, 64u);
    if (!cm) {  // geometry only (device_reflatten): mat, obj and flags stay as khp_set_scene left them
        aux[id].base_d = base_d;
        return;
    }
    const uint32_t m = cm[i];
    if (m >= n_mat) atomicOr(err, 2u);
    aux[id] = Aux{base_d, m, id, 1u};
}

struct LnTable {
    float v[65];
};

// one strand per thread: positions / radii in private memory, then its
// verts-1 cones (khp_gen_hairball followed by khp_fibers_to_cones)
__global__ void k_gen_hairball(uint32_t n, uint32_t verts, float cx, float cy, float cz, float ball_r, float root_r,
                               uint32_t key0, LnTable lnt, float4* base_r0, float4* apex_r1) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    float P[3 * 64], R[64];
    hairball_strand(s, verts, mk(cx, cy, cz), ball_r, root_r, key0, lnt.v, P, R);
    const size_t k0 = (size_t)s * (verts - 1);
    for (uint32_t c = 0; c + 1 < verts; ++c) {
        float ob[4], oa[4];
        fiber_segment(P, R, c, ob, oa);
        base_r0[k0 + c] = make_float4(ob[0], ob[1], ob[2], ob[3]);
        apex_r1[k0 + c] = make_float4(oa[0], oa[1], oa[2], oa[3]);
    }
}

// one triangle per thread: strand s = t / (segs * per_seg) regenerated per
// thread (cheap next to the tube math), then fiber_tube_triangle
__global__ void k_gen_hairball_tris(uint32_t n, uint32_t verts, float cx, float cy, float cz, float ball_r,
                                    float root_r, uint32_t key0, LnTable lnt, uint32_t res, float* ov, float* on,
                                    float* of) {
    const uint32_t per_seg = 2 * res * res, per_strand = (verts - 1) * per_seg;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * per_strand) return;
    const uint32_t s = (uint32_t)(t / per_strand), r = (uint32_t)(t % per_strand);
    float P[3 * 64], R[64];
    hairball_strand(s, verts, mk(cx, cy, cz), ball_r, root_r, key0, lnt.v, P, R);
    fiber_tube_triangle(P, R, r / per_seg, res, r % per_seg, ov + 9 * t, on + 9 * t, of + 9 * t);
}

// ---- fur on a mesh (khp_gen_fur + khp_fibers_to_cones) --------------------------
// Density mode, one face per thread: its fibre count (64-bit, the scan's type).
// err[0] bit 0 / err[1] = the first face whose count would reach 65,536.
__global__ void __launch_bounds__(256)
k_fur_count(const float* __restrict__ tv, uint32_t n_tris, float density, uint32_t key0, uint64_t* cnt,
            uint32_t* err) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_tris) return;
    const float* v = tv + 9 * (size_t)f;
    uint32_t c = fur_face_count(ld3(v), ld3(v + 3), ld3(v + 6), density, fur_face_key(key0, f));
    if (c == FUR_COUNT_BAD) {
        atomicOr(err, 1u);
        atomicMin(err + 1, f);
        c = 0;
    }
    cnt[f] = c;
}

// One fibre per thread (per-face counts vary by orders of magnitude in density
// mode; no lane waits behind a large face).  The strand is streamed: cone c
// needs vertices c and c + 1 only, so nothing but the last vertex is kept.
// first: exclusive prefix of the face counts [n_tris + 1], or null (per_face each).
__global__ void __launch_bounds__(256)
k_gen_fur(khp_fur_params p, uint32_t key0, uint32_t n_tris, uint32_t n_fibers, uint32_t per_face,
          const uint64_t* __restrict__ first, const float* __restrict__ tv, const float* __restrict__ tn, LnTable lnt,
          float4* base_r0, float4* apex_r1) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_fibers) return;
    uint32_t f, j;
    if (first) {  // the face with first[f] <= t < first[f + 1]; first[0] = 0, first[n_tris] = n_fibers > t
        uint32_t lo = 0, hi = n_tris;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (first[mid] <= t) lo = mid;
            else hi = mid;
        }
        f = lo;
        j = t - (uint32_t)first[lo];
    } else {
        f = t / per_face;
        j = t % per_face;
    }
    Strand s = fur_strand_begin(p, key0, f, j, tv + 9 * (size_t)f, tn ? tn + 9 * (size_t)f : nullptr);
    const size_t k0 = (size_t)t * (p.verts - 1);
    for (uint32_t c = 0; c + 1 < p.verts; ++c) {
        const v3 b = s.pos;
        const float br = s.radius;
        strand_next(s, c + 1, lnt.v);
        float ob[4], oa[4];
        fiber_segment_at(b, s.pos, br, s.radius, c, ob, oa);
        base_r0[k0 + c] = make_float4(ob[0], ob[1], ob[2], ob[3]);
        apex_r1[k0 + c] = make_float4(oa[0], oa[1], oa[2], oa[3]);
    }
}

#define FLCHK(expr)                                                                 \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(e_); \
    } while (0)

static uint32_t blocks(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// BSDF kind 11 needs the cone's axis and radius: a triangle whose material is one is refused.
// hair[m]: material m is of that kind.  A material index out of range is k_flatten_tris's to report.
__global__ void k_check_hair_tris(const uint32_t* tm, uint32_t nt, const uint8_t* hair, uint32_t n_mat, uint32_t* err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nt) return;
    const uint32_t m = tm[i];
    if (m < n_mat && hair[m]) atomicOr(err, 128u);
}

// khp_debug_kmath: one item per thread through kmath_ops.h's table, the gfx950 compile of
// what khp_kmath_host loops over.  It lives here and not beside the other queries so that
// no kernel of the render translation unit is compiled next to it.
__global__ void __launch_bounds__(256) k_dbg_kmath(uint32_t op, uint32_t n, const uint64_t* __restrict__ in,
                                                   uint64_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t w[KMATH_WORDS], o[KMATH_WORDS];
    for (int k = 0; k < KMATH_WORDS; ++k) w[k] = in[KMATH_WORDS * (size_t)i + k];
    kmath_apply(op, w, o);
    for (int k = 0; k < KMATH_WORDS; ++k) out[KMATH_WORDS * (size_t)i + k] = o[k];
}

}  // namespace fl

std::string device_kmath(uint32_t op, uint32_t n, const uint64_t* in, uint64_t* out, hipStream_t st) {
    using namespace fl;
    if (const char* why = kmath_args_error(op, n, in, out)) return std::string("EINVAL:khp_debug_kmath: ") + why;
    const size_t bytes = sizeof(uint64_t) * KMATH_WORDS * (size_t)n;
    DevMem din, dout;
    FLCHK(din.ensure(bytes));
    FLCHK(dout.ensure(bytes));
    FLCHK(hipMemcpyAsync(din.p, in, bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_dbg_kmath, dim3(blocks(n, 256)), dim3(256), 0, st, op, n, din.as<uint64_t>(),
                       dout.as<uint64_t>());
    FLCHK(hipGetLastError());
    FLCHK(hipMemcpyAsync(out, dout.p, bytes, hipMemcpyDeviceToHost, st));
    FLCHK(hipStreamSynchronize(st));
    return std::string();
}

std::string device_flatten(const khp_scene* s, bool device_ptrs, uint32_t n_materials, bool textured,
                           const std::vector<float>& models, DeviceObjects& o, hipStream_t st, double* kernel_ms) {
    using namespace fl;
    const uint32_t nt = s->n_tris, nc = s->n_cones, N = nt + nc;
    o.n_obj = N;
    o.n_tris = nt;
    o.n_cones = nc;
    FLCHK(o.rec.ensure(64 * (size_t)N));
    FLCHK(o.aux.ensure(sizeof(Aux) * (size_t)N));
    FLCHK(o.bounds.ensure(24 * (size_t)N));
    FLCHK(o.centroid.ensure(12 * (size_t)N));
    FLCHK(o.tri_nrm.ensure(36 * (size_t)std::max(nt, 1u)));
    FLCHK(o.tri_frame.ensure(36 * (size_t)std::max(nt, 1u)));
    if (s->tri_frame && nt)
        FLCHK(hipMemcpyAsync(o.tri_frame.p, s->tri_frame, 36 * (size_t)nt,
                             device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    else
        FLCHK(hipMemsetAsync(o.tri_frame.p, 0, 36 * (size_t)std::max(nt, 1u), st));
    if (textured) {
        FLCHK(o.tri_uv.ensure(24 * (size_t)std::max(nt, 1u)));
        FLCHK(o.cone_h.ensure(4 * (size_t)std::max(nc, 1u)));
    } else {
        o.tri_uv.release();
        o.cone_h.release();
    }
    DevMem tv, tn, tm, cb, ca, cm, dmodels, err;
    const float *dtv = s->tri_v, *dtn = s->tri_n, *dcb = s->cone_base_r0, *dca = s->cone_apex_r1;
    const float* duv = textured ? s->tri_uv : nullptr;
    const uint32_t *dtm = s->tri_mat, *dcm = s->cone_mat, *dcmod = s->cone_model;
    // the texcoords as the caller gave them stay in HBM: the ctor's reordering follows the
    // vertices, so a later device_reflatten redoes it from the source
    o.tri_uv_src.release();
    if (duv && nt) {
        FLCHK(o.tri_uv_src.ensure(24 * (size_t)nt));
        FLCHK(hipMemcpyAsync(o.tri_uv_src.p, s->tri_uv, 24 * (size_t)nt,
                             device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        duv = o.tri_uv_src.as<float>();
    }
    o.cone_model.release();   // likewise the per-cone model indices of a scene with cone models
    if (!models.empty() && dcmod && nc) {
        FLCHK(o.cone_model.ensure(4 * (size_t)nc));
        FLCHK(hipMemcpyAsync(o.cone_model.p, s->cone_model, 4 * (size_t)nc,
                             device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        dcmod = o.cone_model.as<uint32_t>();
    }
    if (!models.empty()) {
        FLCHK(dmodels.ensure(4 * models.size()));
        FLCHK(hipMemcpyAsync(dmodels.p, models.data(), 4 * models.size(), hipMemcpyHostToDevice, st));
    }
    if (!device_ptrs) {  // the library copies the caller's host arrays (khp_set_scene contract)
        if (nt) {
            FLCHK(tv.ensure(36 * (size_t)nt));
            FLCHK(tn.ensure(36 * (size_t)nt));
            FLCHK(tm.ensure(4 * (size_t)nt));
            FLCHK(hipMemcpyAsync(tv.p, s->tri_v, 36 * (size_t)nt, hipMemcpyHostToDevice, st));
            FLCHK(hipMemcpyAsync(tn.p, s->tri_n, 36 * (size_t)nt, hipMemcpyHostToDevice, st));
            FLCHK(hipMemcpyAsync(tm.p, s->tri_mat, 4 * (size_t)nt, hipMemcpyHostToDevice, st));
            dtv = tv.as<float>();
            dtn = tn.as<float>();
            dtm = tm.as<uint32_t>();
        }
        if (nc) {
            FLCHK(cb.ensure(16 * (size_t)nc));
            FLCHK(ca.ensure(16 * (size_t)nc));
            FLCHK(cm.ensure(4 * (size_t)nc));
            FLCHK(hipMemcpyAsync(cb.p, s->cone_base_r0, 16 * (size_t)nc, hipMemcpyHostToDevice, st));
            FLCHK(hipMemcpyAsync(ca.p, s->cone_apex_r1, 16 * (size_t)nc, hipMemcpyHostToDevice, st));
            FLCHK(hipMemcpyAsync(cm.p, s->cone_mat, 4 * (size_t)nc, hipMemcpyHostToDevice, st));
            dcb = cb.as<float>();
            dca = ca.as<float>();
            dcm = cm.as<uint32_t>();
        }
    }
    FLCHK(err.ensure(4));
    FLCHK(hipMemsetAsync(err.p, 0, 4, st));
    hipEvent_t e0, e1;
    FLCHK(hipEventCreate(&e0));
    FLCHK(hipEventCreate(&e1));
    FLCHK(hipEventRecord(e0, st));
    if (nt)
        hipLaunchKernelGGL(k_flatten_tris, dim3(blocks(nt, 256)), dim3(256), 0, st, dtv, dtn, dtm, duv, nt,
                           n_materials, o.rec.as<float4>(), o.aux.as<Aux>(), o.bounds.as<float>(),
                           o.centroid.as<float>(), o.tri_nrm.as<float>(), textured ? o.tri_uv.as<float>() : nullptr,
                           err.as<uint32_t>());
    if (nc)
        hipLaunchKernelGGL(k_flatten_cones, dim3(blocks(nc, 256)), dim3(256), 0, st, (const float4*)dcb,
                           (const float4*)dca, dcm, models.empty() ? nullptr : dcmod,
                           models.empty() ? nullptr : dmodels.as<float>(), (uint32_t)(models.size() / 25), nc, nt,
                           n_materials, o.rec.as<float4>(), o.aux.as<Aux>(), o.bounds.as<float>(),
                           o.centroid.as<float>(), textured ? o.cone_h.as<float>() : nullptr, err.as<uint32_t>());
    FLCHK(hipGetLastError());
    DevMem dhair;
    if (nt) {   // next to the material-index check: no triangle of a ChiangHairBSDF material
        std::vector<uint8_t> hair(n_materials, 0);
        bool any = false;
        for (uint32_t m = 0; m < n_materials; ++m) any |= (hair[m] = s->materials[m].bsdf == KHP_BSDF_CHIANG_HAIR) != 0;
        if (any) {
            FLCHK(dhair.ensure(hair.size()));
            FLCHK(hipMemcpyAsync(dhair.p, hair.data(), hair.size(), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_check_hair_tris, dim3(blocks(nt, 256)), dim3(256), 0, st, dtm, nt, dhair.as<uint8_t>(),
                               n_materials, err.as<uint32_t>());
            FLCHK(hipGetLastError());
        }
    }
    FLCHK(hipEventRecord(e1, st));
    uint32_t herr = 0;
    FLCHK(hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, st));
    FLCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    FLCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (kernel_ms) *kernel_ms = ms;
    if (herr & 1u) return "EINVAL:triangle material index out of range";
    if (herr & 2u) return "EINVAL:cone material index out of range";
    if (herr & 4u) return "EINVAL:cone model index out of range";
    if (herr & 8u) return "EINVAL:tri_v holds a NaN or an infinity";
    if (herr & 16u) return "EINVAL:cone_base_r0 holds a NaN or an infinity";
    if (herr & 32u) return "EINVAL:cone_apex_r1 holds a NaN or an infinity";
    if (herr & 64u) return "EINVAL:an object's bounds or centroid overflow float32";
    if (herr & 128u) return "EINVAL:a triangle's material is a ChiangHairBSDF: the kind needs a cone's axis and radius";
    return std::string();
}

std::string device_reflatten(const khp_scene* s, bool device_ptrs, bool textured, const std::vector<float>& models,
                             DeviceObjects& o, hipStream_t st, double* kernel_ms) {
    using namespace fl;
    const uint32_t nt = o.n_tris, nc = o.n_cones;  // the caller checked s->n_tris / s->n_cones against them
    if (s->tri_frame && nt)
        FLCHK(hipMemcpyAsync(o.tri_frame.p, s->tri_frame, 36 * (size_t)nt,
                             device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    else
        FLCHK(hipMemsetAsync(o.tri_frame.p, 0, 36 * (size_t)std::max(nt, 1u), st));
    DevMem tv, tn, cb, ca, dmodels, err;
    const float *dtv = s->tri_v, *dtn = s->tri_n, *dcb = s->cone_base_r0, *dca = s->cone_apex_r1;
    if (!models.empty()) {
        FLCHK(dmodels.ensure(4 * models.size()));
        FLCHK(hipMemcpyAsync(dmodels.p, models.data(), 4 * models.size(), hipMemcpyHostToDevice, st));
    }
    if (!device_ptrs) {
        if (nt) {
            FLCHK(tv.ensure(36 * (size_t)nt));
            FLCHK(tn.ensure(36 * (size_t)nt));
            FLCHK(hipMemcpyAsync(tv.p, s->tri_v, 36 * (size_t)nt, hipMemcpyHostToDevice, st));
            FLCHK(hipMemcpyAsync(tn.p, s->tri_n, 36 * (size_t)nt, hipMemcpyHostToDevice, st));
            dtv = tv.as<float>();
            dtn = tn.as<float>();
        }
        if (nc) {
            FLCHK(cb.ensure(16 * (size_t)nc));
            FLCHK(ca.ensure(16 * (size_t)nc));
            FLCHK(hipMemcpyAsync(cb.p, s->cone_base_r0, 16 * (size_t)nc, hipMemcpyHostToDevice, st));
            FLCHK(hipMemcpyAsync(ca.p, s->cone_apex_r1, 16 * (size_t)nc, hipMemcpyHostToDevice, st));
            dcb = cb.as<float>();
            dca = ca.as<float>();
        }
    }
    FLCHK(err.ensure(4));
    FLCHK(hipMemsetAsync(err.p, 0, 4, st));
    hipEvent_t e0, e1;
    FLCHK(hipEventCreate(&e0));
    FLCHK(hipEventCreate(&e1));
    FLCHK(hipEventRecord(e0, st));
    if (nt)
        hipLaunchKernelGGL(k_flatten_tris, dim3(blocks(nt, 256)), dim3(256), 0, st, dtv, dtn, (const uint32_t*)nullptr,
                           (const float*)o.tri_uv_src.as<float>(), nt, 0u, o.rec.as<float4>(), o.aux.as<Aux>(),
                           o.bounds.as<float>(), o.centroid.as<float>(), o.tri_nrm.as<float>(),
                           textured ? o.tri_uv.as<float>() : nullptr, err.as<uint32_t>());
    if (nc)
        hipLaunchKernelGGL(k_flatten_cones, dim3(blocks(nc, 256)), dim3(256), 0, st, (const float4*)dcb,
                           (const float4*)dca, (const uint32_t*)nullptr,
                           models.empty() ? nullptr : (const uint32_t*)o.cone_model.as<uint32_t>(),
                           models.empty() ? nullptr : (const float*)dmodels.as<float>(), (uint32_t)(models.size() / 25),
                           nc, nt, 0u, o.rec.as<float4>(), o.aux.as<Aux>(), o.bounds.as<float>(),
                           o.centroid.as<float>(), textured ? o.cone_h.as<float>() : nullptr, err.as<uint32_t>());
    FLCHK(hipGetLastError());
    FLCHK(hipEventRecord(e1, st));
    uint32_t herr = 0;
    FLCHK(hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, st));
    FLCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    FLCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (kernel_ms) *kernel_ms = ms;
    if (herr & 8u) return "EINVAL:tri_v holds a NaN or an infinity";
    if (herr & 16u) return "EINVAL:cone_base_r0 holds a NaN or an infinity";
    if (herr & 32u) return "EINVAL:cone_apex_r1 holds a NaN or an infinity";
    if (herr & 64u) return "EINVAL:an object's bounds or centroid overflow float32";
    return std::string();
}

std::string device_gen_hairball(uint32_t n, uint32_t verts, const float center[3], float ball_r, float root_r,
                                uint32_t seed, float* d_base_r0, float* d_apex_r1, hipStream_t st) {
    using namespace fl;
    LnTable t{};
    for (int i = 1; i <= 64; ++i) t.v[i] = (float)std::log((double)i);  // as khp_gen_hairball
    const uint32_t key0 = lowbias32(seed ^ 0x48414952u);
    if (n)
        hipLaunchKernelGGL(k_gen_hairball, dim3(blocks(n, 128)), dim3(128), 0, st, n, verts, center[0], center[1],
                           center[2], ball_r, root_r, key0, t, (float4*)d_base_r0, (float4*)d_apex_r1);
    FLCHK(hipGetLastError());
    FLCHK(hipStreamSynchronize(st));
    return std::string();
}

std::string device_gen_fur(const khp_fur_params* p, uint32_t n_tris, const float* d_tri_v, const float* d_tri_n,
                           uint64_t capacity_cones, float* d_base_r0, float* d_apex_r1, uint64_t* n_cones,
                           hipStream_t st) {
    using namespace fl;
    std::string perr = fur_params_error(p);
    if (!perr.empty()) return "EINVAL:" + perr;
    if (!n_cones) return "EINVAL:fur: n_cones is null";
    const bool dens = p->density > 0.0f;
    if (n_tris && !d_tri_v && (dens || d_base_r0)) return "EINVAL:fur: d_tri_v is null";
    if (n_tris >= 0x7fffffffu) return "EINVAL:fur: more than 2^31 - 2 faces";  // the scan counts in int
    const uint32_t key0 = fur_key0(p->seed);
    DevMem cnt, first, err, tmp;
    uint64_t n_fibers = (uint64_t)n_tris * p->fibers_per_face;
    if (dens && n_tris) {
        const int items = (int)n_tris + 1;
        FLCHK(cnt.ensure(8 * (size_t)items));
        FLCHK(first.ensure(8 * (size_t)items));
        FLCHK(err.ensure(8));
        size_t tbytes = 0;
        FLCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tbytes, (uint64_t*)nullptr, (uint64_t*)nullptr, items, st));
        FLCHK(tmp.ensure(tbytes));
        const uint32_t err0[2] = {0u, 0xFFFFFFFFu};
        FLCHK(hipMemcpyAsync(err.p, err0, 8, hipMemcpyHostToDevice, st));
        FLCHK(hipMemsetAsync(cnt.as<uint64_t>() + n_tris, 0, 8, st));
        hipLaunchKernelGGL(k_fur_count, dim3(blocks(n_tris, 256)), dim3(256), 0, st, d_tri_v, n_tris, p->density, key0,
                           cnt.as<uint64_t>(), err.as<uint32_t>());
        FLCHK(hipGetLastError());
        tbytes = tmp.bytes;
        FLCHK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tbytes, cnt.as<uint64_t>(), first.as<uint64_t>(), items, st));
        uint32_t herr[2] = {0, 0};
        FLCHK(hipMemcpyAsync(&n_fibers, first.as<uint64_t>() + n_tris, 8, hipMemcpyDeviceToHost, st));
        FLCHK(hipMemcpyAsync(herr, err.p, 8, hipMemcpyDeviceToHost, st));
        FLCHK(hipStreamSynchronize(st));
        if (herr[0] & 1u) return "EINVAL:fur: face " + std::to_string(herr[1]) + ": fibre count reaches 65536";
    } else if (dens) {
        n_fibers = 0;
    }
    perr = fur_total_error(n_fibers, p->verts, n_tris);
    if (!perr.empty()) return "EINVAL:" + perr;
    *n_cones = n_fibers * (p->verts - 1);
    if (!d_base_r0) return std::string();  // the count only
    if (!d_apex_r1 || (!d_tri_n && p->frame == KHP_FUR_FRAME_NORMAL && n_fibers))
        return "EINVAL:fur: null array";
    if (capacity_cones < *n_cones) return "EINVAL:fur: capacity_cones is smaller than the cone count";
    if (n_fibers) {
        LnTable t{};
        const float* ln = fur_ln_table();
        for (int i = 0; i <= 64; ++i) t.v[i] = ln[i];
        hipLaunchKernelGGL(k_gen_fur, dim3(blocks(n_fibers, 256)), dim3(256), 0, st, *p, key0, n_tris,
                           (uint32_t)n_fibers, p->fibers_per_face, dens ? first.as<uint64_t>() : nullptr, d_tri_v,
                           d_tri_n, t, (float4*)d_base_r0, (float4*)d_apex_r1);
        FLCHK(hipGetLastError());
        FLCHK(hipStreamSynchronize(st));
    }
    return std::string();
}

std::string device_gen_hairball_tris(uint32_t n, uint32_t verts, const float center[3], float ball_r, float root_r,
                                     uint32_t seed, uint32_t res, float* d_v, float* d_n, float* d_frame,
                                     hipStream_t st) {
    using namespace fl;
    LnTable t{};
    for (int i = 1; i <= 64; ++i) t.v[i] = (float)std::log((double)i);
    const uint32_t key0 = lowbias32(seed ^ 0x48414952u);
    const size_t nt = (size_t)n * (verts - 1) * 2 * res * res;
    if (nt)
        hipLaunchKernelGGL(k_gen_hairball_tris, dim3((uint32_t)((nt + 127) / 128)), dim3(128), 0, st, n, verts,
                           center[0], center[1], center[2], ball_r, root_r, key0, t, res, d_v, d_n, d_frame);
    FLCHK(hipGetLastError());
    FLCHK(hipStreamSynchronize(st));
    return std::string();
}

}  // namespace khp
