// debug_query.h -- ABI 15 / 16 batch queries of the shading functions (test hooks,
// included by render.hip next to khp_debug_queue).  Each kernel runs one item
// per thread in a grid-stride loop and calls the __device__ functions the
// renderer calls -- trace_closest, surface_at, bsdf_sample<KINDS>, bsdf_eval,
// light_dir, light_isect, light_emit, and (ABI 16) bsdf_sample's KINDS_LOBES
// instance, hair_lobes.h -- so a test can compare them item by item
// with the oracle and with a float64 reference.  ABI 17 adds the light-path
// variant's: k_light_paths itself, bd_connection and img_connection; after them come
// the texture lookups': tex_color, env_color and hit_texcoord / resolve_material (at the end).
// Every index is checked on the host before a launch; the kernels read nothing
// the host has not validated.
#pragma once

constexpr uint32_t DBG_MAX_ITEMS = 1u << 20;
constexpr uint32_t DBG_BLOCK = 256;
static uint32_t dbg_grid(uint32_t n) { return std::min((n + DBG_BLOCK - 1) / DBG_BLOCK, 1024u); }

__device__ __forceinline__ void st3(float* d, v3 a) {
    d[0] = a.x;
    d[1] = a.y;
    d[2] = a.z;
}

template <bool TEX>
__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_surface(DevScene S, uint32_t n, const float* orig, const float* dir,
                                                           float* t_out, int32_t* obj_out, float* nrm, float* uvw,
                                                           int32_t* mat) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Ray r = make_ray(ld3(orig + 3 * (size_t)i), ld3(dir + 3 * (size_t)i));
        Hit h;
        PrivStack stk;
        TravStats st{0, 0};
        trace_closest<false>(S, r, h, stk, st);
        const v3 zero = mk(0.0f, 0.0f, 0.0f);
        ShadeCtx s;
        s.U = s.V = s.W = zero;
        v3 nn = zero;
        int32_t m = -1, ob = -1;
        if (h.slot >= 0) {
            khp_material mres;
            nn = surface_at<TEX>(S, r, h, s, mres);
            const Aux ax = S.aux[h.slot];
            m = (int32_t)ax.mat;
            ob = (int32_t)ax.obj;
        }
        t_out[i] = h.t;
        obj_out[i] = ob;
        st3(nrm + 3 * (size_t)i, nn);
        st3(uvw + 9 * (size_t)i, s.U);
        st3(uvw + 9 * (size_t)i + 3, s.V);
        st3(uvw + 9 * (size_t)i + 6, s.W);
        mat[i] = m;
    }
}

// The hair frame of the object in `slot`, as surface_at loads it: the cone
// record's rows, or the triangle's tri_frame entry.
__device__ __forceinline__ void dbg_frame(const DevScene& S, uint32_t slot, ShadeCtx& s) {
    const Aux ax = S.aux[slot];
    if (ax.flags & 1u) {
        const float4* pr = S.prims + 4 * (size_t)slot;
        const float4 c1 = pr[1], c2 = pr[2], c3 = pr[3];
        s.U = mk(c1.x, c1.y, c1.z);
        s.V = mk(c2.x, c2.y, c2.z);
        s.W = mk(c3.x, c3.y, c3.z);
    } else {
        const float* tf = S.tri_frame + 9 * (size_t)ax.obj;
        s.U = ld3(tf);
        s.V = ld3(tf + 3);
        s.W = ld3(tf + 6);
    }
}

template <uint32_t KINDS>
__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_bsdf_sample(DevScene S, uint32_t n, const uint32_t* slot,
                                                               const int32_t* mat, const float* in, const float* nrm,
                                                               const float* sample, const float* hair,
                                                               const int32_t* flags_in, float* out_dir, float* pdf,
                                                               float* f, float* sample_out, int32_t* flags_out,
                                                               int32_t* valid) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        ShadeCtx s;
        dbg_frame(S, slot[i], s);
        s.m = &S.mats[mat[i]];
        s.n = ld3(nrm + 3 * (size_t)i);
        float sm[2] = {sample[2 * (size_t)i], sample[2 * (size_t)i + 1]};
        v3 out = mk(0.0f, 0.0f, 0.0f);
        float pd = 0.0f;
        int flags = flags_in[i];
        bool ok = false;
        const v3 r = bsdf_sample<KINDS>(s, ld3(in + 3 * (size_t)i), s.n, sm, hair[2 * (size_t)i],
                                        hair[2 * (size_t)i + 1], out, pd, flags, ok);
        st3(out_dir + 3 * (size_t)i, out);
        st3(f + 3 * (size_t)i, r);
        pdf[i] = pd;
        sample_out[2 * (size_t)i] = sm[0];
        sample_out[2 * (size_t)i + 1] = sm[1];
        flags_out[i] = flags;
        valid[i] = ok ? 1 : 0;
    }
}

// ABI 16: bsdf_sample of a KINDS_LOBES instance (hair_lobes.h) with the lobe set and draw of the call.
__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_hair_sample(DevScene S, uint32_t n, uint32_t lobes, const uint32_t* slot,
                                                               const int32_t* mat, const float* in, const float* nrm,
                                                               const float* hair, const float* lobe_u,
                                                               const int32_t* flags_in, float* out_dir, float* pdf,
                                                               float* f, float* sample_out, int32_t* flags_out,
                                                               int32_t* valid) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        ShadeCtx s;
        dbg_frame(S, slot[i], s);
        s.m = &S.mats[mat[i]];
        s.n = ld3(nrm + 3 * (size_t)i);
        float sm[2] = {0.0f, 0.0f};
        v3 out = mk(0.0f, 0.0f, 0.0f);
        float pd = 0.0f;
        int flags = flags_in[i];
        bool ok = false;
        const v3 r = bsdf_sample<KINDS_FUR | KINDS_LOBES>(s, ld3(in + 3 * (size_t)i), s.n, sm, hair[2 * (size_t)i],
                                                          hair[2 * (size_t)i + 1], out, pd, flags, ok, lobe_u[i], lobes);
        st3(out_dir + 3 * (size_t)i, out);
        st3(f + 3 * (size_t)i, r);
        pdf[i] = pd;
        sample_out[2 * (size_t)i] = sm[0];
        sample_out[2 * (size_t)i + 1] = sm[1];
        flags_out[i] = flags;
        valid[i] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_bsdf_eval(DevScene S, uint32_t n, const uint32_t* slot,
                                                             const int32_t* mat, const float* in, const float* nrm,
                                                             const float* out, float* f) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        ShadeCtx s;
        dbg_frame(S, slot[i], s);
        s.m = &S.mats[mat[i]];
        s.n = ld3(nrm + 3 * (size_t)i);
        st3(f + 3 * (size_t)i, bsdf_eval(s, ld3(in + 3 * (size_t)i), ld3(out + 3 * (size_t)i)));
    }
}

// The same with BSDF kind 11 compiled in (hair_pb.h): launched when an item is of that kind.
__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_bsdf_eval_hair(DevScene S, uint32_t n, const uint32_t* slot,
                                                                  const int32_t* mat, const float* in, const float* nrm,
                                                                  const float* out, float* f) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        ShadeCtx s;
        dbg_frame(S, slot[i], s);
        s.m = &S.mats[mat[i]];
        s.n = ld3(nrm + 3 * (size_t)i);
        st3(f + 3 * (size_t)i, bsdf_eval<KINDS_ALL_HAIR>(s, ld3(in + 3 * (size_t)i), ld3(out + 3 * (size_t)i)));
    }
}

__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_light_dir(DevScene S, uint32_t n, const int32_t* li, const float* p,
                                                             const float* u, float* ro, float* rd, float* att) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const DevLight L = S.lights[li[i]];
        float a = 0.0f;
        const Ray r = light_dir(L, ld3(p + 3 * (size_t)i), u[2 * (size_t)i], u[2 * (size_t)i + 1], a);
        st3(ro + 3 * (size_t)i, r.o);
        st3(rd + 3 * (size_t)i, r.d);
        att[i] = a;
    }
}

__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_light_isect(DevScene S, uint32_t n, const int32_t* li,
                                                               const float* orig, const float* dir, uint8_t* hit,
                                                               float* t_out, float* emit) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const DevLight L = S.lights[li[i]];
        const Ray r = make_ray(ld3(orig + 3 * (size_t)i), ld3(dir + 3 * (size_t)i));
        float t = 0.0f;
        const bool h = light_isect(L, r, t);
        hit[i] = h ? 1 : 0;
        t_out[i] = h ? t : 0.0f;
        st3(emit + 3 * (size_t)i, light_emit(L, r.d));
    }
}

// ---- host side ---------------------------------------------------------------------------
static khp_status dbg_enter(khp_ctx* c, uint32_t n, bool ptrs_ok) {
    if (!c) return fail(KHP_EINVAL, "ctx is null");
    KHPCHK(drain(c));  // complete asynchronous frames first
    if (!ptrs_ok) return fail(KHP_EINVAL, "null argument");
    if (n == 0 || n > DBG_MAX_ITEMS) return fail(KHP_EINVAL, "n must be in [1, 2^20]");
    if (!c->scene_set) return fail(KHP_ENOTREADY, "khp_set_scene first");
    if (!c->built) return fail(KHP_ENOTREADY, "khp_build_accel first");
    HIPCHK(hipSetDevice(c->device));
    return KHP_OK;
}

// The slot of every object (object-id order), from the layout in HBM.
static khp_status dbg_object_slots(khp_ctx* c, std::vector<uint32_t>& slot_of) {
    std::vector<Aux> aux(c->n_slots);
    std::vector<float4> prims(4 * (size_t)c->n_slots);
    if (c->n_slots) {
        HIPCHK(hipMemcpyAsync(aux.data(), c->aux.p, sizeof(Aux) * aux.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(prims.data(), c->prims.p, sizeof(float4) * prims.size(), hipMemcpyDeviceToHost, c->stream));
        KHPCHK(wait_stream(c, c->stream, "the layout read"));
    }
    slot_of.assign(c->hs.n_obj, UINT32_MAX);
    for (uint32_t s = 0; s < c->n_slots; ++s) {
        uint32_t tag;
        memcpy(&tag, &prims[4 * (size_t)s].w, sizeof(tag));
        const bool real = (aux[s].flags & 1u) || tag == TRI_TAG;   // pad slots are zero records
        if (real && aux[s].obj < slot_of.size()) slot_of[aux[s].obj] = s;
    }
    return KHP_OK;
}

// Validates the (object, material) items of a BSDF query and resolves the objects' slots.
static khp_status dbg_bsdf_items(khp_ctx* c, uint32_t n, const int32_t* obj, const int32_t* mat, uint32_t kinds_mask,
                                 std::vector<uint32_t>& slots) {
    if (kinds_mask != KINDS_ALL && kinds_mask != KINDS_FUR && kinds_mask != KINDS_ALL_HAIR && kinds_mask != KINDS_FUR_HAIR)
        return fail(KHP_EINVAL, "kinds_mask must be the full set or the fur set (Lambert + Marschner), or, with "
                                "ChiangHairBSDF, the twelve kinds or Lambert + ChiangHairBSDF");
    std::vector<uint32_t> slot_of;
    KHPCHK(dbg_object_slots(c, slot_of));
    slots.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (obj[i] < 0 || (uint32_t)obj[i] >= slot_of.size() || slot_of[obj[i]] == UINT32_MAX)
            return fail(KHP_EINVAL, "item " + std::to_string(i) + ": object id out of range");
        if (mat[i] < 0 || (size_t)mat[i] >= c->hs.mats.size())
            return fail(KHP_EINVAL, "item " + std::to_string(i) + ": material index out of range");
        const int32_t k = c->hs.mats[mat[i]].bsdf;
        const uint32_t bit = (k >= 0 && k < KHP_BSDF_COUNT) ? (1u << k) : KINDS_ALL_HAIR;
        if (bit & ~kinds_mask)   // the instance has this case compiled out: never launch
            return fail(KHP_EINVAL, "item " + std::to_string(i) + ": BSDF kind " + std::to_string(k) +
                                        " is outside kinds_mask");
        slots[i] = slot_of[obj[i]];
    }
    return KHP_OK;
}

extern "C" khp_status khp_debug_surface(khp_ctx* c, uint32_t n, const float* orig, const float* dir, float* t_out,
                                        int32_t* obj_out, float* normal, float* uvw, int32_t* mat_out) {
    KHPCHK(dbg_enter(c, n, orig && dir && t_out && obj_out && normal && uvw && mat_out));
    DevMem o, d, t, ob, nr, fr, mt;
    HIPCHK(upload(o, orig, 3 * (size_t)n, c->stream));
    HIPCHK(upload(d, dir, 3 * (size_t)n, c->stream));
    HIPCHK(t.ensure(4 * (size_t)n));
    HIPCHK(ob.ensure(4 * (size_t)n));
    HIPCHK(nr.ensure(12 * (size_t)n));
    HIPCHK(fr.ensure(36 * (size_t)n));
    HIPCHK(mt.ensure(4 * (size_t)n));
    if (c->S.textured)
        hipLaunchKernelGGL(k_dbg_surface<true>, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n, o.as<float>(),
                           d.as<float>(), t.as<float>(), ob.as<int32_t>(), nr.as<float>(), fr.as<float>(), mt.as<int32_t>());
    else
        hipLaunchKernelGGL(k_dbg_surface<false>, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n, o.as<float>(),
                           d.as<float>(), t.as<float>(), ob.as<int32_t>(), nr.as<float>(), fr.as<float>(), mt.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(t_out, t.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(obj_out, ob.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(normal, nr.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(uvw, fr.p, 36 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(mat_out, mt.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the surface queries"));
    return KHP_OK;
}

extern "C" khp_status khp_debug_bsdf_sample(khp_ctx* c, uint32_t n, uint32_t kinds_mask, const int32_t* obj,
                                            const int32_t* mat, const float* in, const float* normal,
                                            const float* sample, const float* hair, const int32_t* flags_in,
                                            float* out_dir, float* pdf, float* f, float* sample_out,
                                            int32_t* flags_out, int32_t* valid) {
    KHPCHK(dbg_enter(c, n, obj && mat && in && normal && sample && hair && flags_in && out_dir && pdf && f &&
                               sample_out && flags_out && valid));
    std::vector<uint32_t> slots;
    KHPCHK(dbg_bsdf_items(c, n, obj, mat, kinds_mask, slots));
    DevMem sl, mt, di, dn, ds, dh, dfl, od, op, of, os, ofl, ov;
    HIPCHK(upload(sl, slots.data(), (size_t)n, c->stream));
    HIPCHK(upload(mt, mat, (size_t)n, c->stream));
    HIPCHK(upload(di, in, 3 * (size_t)n, c->stream));
    HIPCHK(upload(dn, normal, 3 * (size_t)n, c->stream));
    HIPCHK(upload(ds, sample, 2 * (size_t)n, c->stream));
    HIPCHK(upload(dh, hair, 2 * (size_t)n, c->stream));
    HIPCHK(upload(dfl, flags_in, (size_t)n, c->stream));
    HIPCHK(od.ensure(12 * (size_t)n));
    HIPCHK(op.ensure(4 * (size_t)n));
    HIPCHK(of.ensure(12 * (size_t)n));
    HIPCHK(os.ensure(8 * (size_t)n));
    HIPCHK(ofl.ensure(4 * (size_t)n));
    HIPCHK(ov.ensure(4 * (size_t)n));
    if (kinds_mask == KINDS_ALL_HAIR || kinds_mask == KINDS_FUR_HAIR)   // one covering instance, as the renderer's
        hipLaunchKernelGGL(k_dbg_bsdf_sample<KINDS_ALL_HAIR>, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n,
                           sl.as<uint32_t>(), mt.as<int32_t>(), di.as<float>(), dn.as<float>(), ds.as<float>(),
                           dh.as<float>(), dfl.as<int32_t>(), od.as<float>(), op.as<float>(), of.as<float>(),
                           os.as<float>(), ofl.as<int32_t>(), ov.as<int32_t>());
    else if (kinds_mask == KINDS_FUR)
        hipLaunchKernelGGL(k_dbg_bsdf_sample<KINDS_FUR>, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n,
                           sl.as<uint32_t>(), mt.as<int32_t>(), di.as<float>(), dn.as<float>(), ds.as<float>(),
                           dh.as<float>(), dfl.as<int32_t>(), od.as<float>(), op.as<float>(), of.as<float>(),
                           os.as<float>(), ofl.as<int32_t>(), ov.as<int32_t>());
    else
        hipLaunchKernelGGL(k_dbg_bsdf_sample<KINDS_ALL>, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n,
                           sl.as<uint32_t>(), mt.as<int32_t>(), di.as<float>(), dn.as<float>(), ds.as<float>(),
                           dh.as<float>(), dfl.as<int32_t>(), od.as<float>(), op.as<float>(), of.as<float>(),
                           os.as<float>(), ofl.as<int32_t>(), ov.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_dir, od.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pdf, op.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(f, of.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(sample_out, os.p, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(flags_out, ofl.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(valid, ov.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the BSDF queries"));
    return KHP_OK;
}

extern "C" khp_status khp_debug_hair_sample(khp_ctx* c, uint32_t n, uint32_t lobes, const int32_t* obj,
                                            const int32_t* mat, const float* in, const float* normal,
                                            const float* hair, const float* lobe_u, const int32_t* flags_in,
                                            float* out_dir, float* pdf, float* f, float* sample_out,
                                            int32_t* flags_out, int32_t* valid) {
    KHPCHK(dbg_enter(c, n, obj && mat && in && normal && hair && lobe_u && flags_in && out_dir && pdf && f &&
                               sample_out && flags_out && valid));
    if (lobes == 0u || (lobes & ~HAIR_LOBE_ALL))
        return fail(KHP_EINVAL, "lobes must be a non-empty set of KHP_HAIR_LOBE_R, _TT, _TRT");
    std::vector<uint32_t> slots;
    KHPCHK(dbg_bsdf_items(c, n, obj, mat, KINDS_ALL, slots));
    for (uint32_t i = 0; i < n; ++i)
        if (c->hs.mats[mat[i]].bsdf != KHP_BSDF_MARSCHNER_HAIR)
            return fail(KHP_EINVAL, "item " + std::to_string(i) + ": material " + std::to_string(mat[i]) +
                                        " is not KHP_BSDF_MARSCHNER_HAIR");
    DevMem sl, mt, di, dn, dh, du, dfl, od, op, of, os, ofl, ov;
    HIPCHK(upload(sl, slots.data(), (size_t)n, c->stream));
    HIPCHK(upload(mt, mat, (size_t)n, c->stream));
    HIPCHK(upload(di, in, 3 * (size_t)n, c->stream));
    HIPCHK(upload(dn, normal, 3 * (size_t)n, c->stream));
    HIPCHK(upload(dh, hair, 2 * (size_t)n, c->stream));
    HIPCHK(upload(du, lobe_u, (size_t)n, c->stream));
    HIPCHK(upload(dfl, flags_in, (size_t)n, c->stream));
    HIPCHK(od.ensure(12 * (size_t)n));
    HIPCHK(op.ensure(4 * (size_t)n));
    HIPCHK(of.ensure(12 * (size_t)n));
    HIPCHK(os.ensure(8 * (size_t)n));
    HIPCHK(ofl.ensure(4 * (size_t)n));
    HIPCHK(ov.ensure(4 * (size_t)n));
    hipLaunchKernelGGL(k_dbg_hair_sample, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n, lobes,
                       sl.as<uint32_t>(), mt.as<int32_t>(), di.as<float>(), dn.as<float>(), dh.as<float>(),
                       du.as<float>(), dfl.as<int32_t>(), od.as<float>(), op.as<float>(), of.as<float>(),
                       os.as<float>(), ofl.as<int32_t>(), ov.as<int32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_dir, od.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pdf, op.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(f, of.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(sample_out, os.p, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(flags_out, ofl.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(valid, ov.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the BSDF queries"));
    return KHP_OK;
}

extern "C" khp_status khp_debug_bsdf_eval(khp_ctx* c, uint32_t n, const int32_t* obj, const int32_t* mat,
                                          const float* in, const float* normal, const float* out, float* f) {
    KHPCHK(dbg_enter(c, n, obj && mat && in && normal && out && f));
    std::vector<uint32_t> slots;
    KHPCHK(dbg_bsdf_items(c, n, obj, mat, KINDS_ALL_HAIR, slots));
    bool hair = false;
    for (uint32_t i = 0; i < n; ++i) hair = hair || c->hs.mats[mat[i]].bsdf == KHP_BSDF_CHIANG_HAIR;
    DevMem sl, mt, di, dn, dout, of;
    HIPCHK(upload(sl, slots.data(), (size_t)n, c->stream));
    HIPCHK(upload(mt, mat, (size_t)n, c->stream));
    HIPCHK(upload(di, in, 3 * (size_t)n, c->stream));
    HIPCHK(upload(dn, normal, 3 * (size_t)n, c->stream));
    HIPCHK(upload(dout, out, 3 * (size_t)n, c->stream));
    HIPCHK(of.ensure(12 * (size_t)n));
    if (hair)
        hipLaunchKernelGGL(k_dbg_bsdf_eval_hair, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n,
                           sl.as<uint32_t>(), mt.as<int32_t>(), di.as<float>(), dn.as<float>(), dout.as<float>(),
                           of.as<float>());
    else
        hipLaunchKernelGGL(k_dbg_bsdf_eval, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n, sl.as<uint32_t>(),
                           mt.as<int32_t>(), di.as<float>(), dn.as<float>(), dout.as<float>(), of.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(f, of.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the BSDF queries"));
    return KHP_OK;
}

static khp_status dbg_light_items(khp_ctx* c, uint32_t n, const int32_t* light) {
    for (uint32_t i = 0; i < n; ++i)
        if (light[i] < 0 || (size_t)light[i] >= c->hs.lights.size())
            return fail(KHP_EINVAL, "item " + std::to_string(i) + ": light index out of range");
    return KHP_OK;
}

extern "C" khp_status khp_debug_light_dir(khp_ctx* c, uint32_t n, const int32_t* light, const float* point,
                                          const float* draws, float* ray_orig, float* ray_dir, float* att) {
    KHPCHK(dbg_enter(c, n, light && point && draws && ray_orig && ray_dir && att));
    KHPCHK(dbg_light_items(c, n, light));
    DevMem dl, dp, du, ro, rd, at;
    HIPCHK(upload(dl, light, (size_t)n, c->stream));
    HIPCHK(upload(dp, point, 3 * (size_t)n, c->stream));
    HIPCHK(upload(du, draws, 2 * (size_t)n, c->stream));
    HIPCHK(ro.ensure(12 * (size_t)n));
    HIPCHK(rd.ensure(12 * (size_t)n));
    HIPCHK(at.ensure(4 * (size_t)n));
    hipLaunchKernelGGL(k_dbg_light_dir, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n, dl.as<int32_t>(),
                       dp.as<float>(), du.as<float>(), ro.as<float>(), rd.as<float>(), at.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ray_orig, ro.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ray_dir, rd.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(att, at.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the light queries"));
    return KHP_OK;
}

extern "C" khp_status khp_debug_light_isect(khp_ctx* c, uint32_t n, const int32_t* light, const float* orig,
                                            const float* dir, uint8_t* hit, float* t_out, float* emit) {
    KHPCHK(dbg_enter(c, n, light && orig && dir && hit && t_out && emit));
    KHPCHK(dbg_light_items(c, n, light));
    DevMem dl, o, d, dh, dt, de;
    HIPCHK(upload(dl, light, (size_t)n, c->stream));
    HIPCHK(upload(o, orig, 3 * (size_t)n, c->stream));
    HIPCHK(upload(d, dir, 3 * (size_t)n, c->stream));
    HIPCHK(dh.ensure((size_t)n));
    HIPCHK(dt.ensure(4 * (size_t)n));
    HIPCHK(de.ensure(12 * (size_t)n));
    hipLaunchKernelGGL(k_dbg_light_isect, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n, dl.as<int32_t>(),
                       o.as<float>(), d.as<float>(), dh.as<uint8_t>(), dt.as<float>(), de.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hit, dh.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(t_out, dt.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(emit, de.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the light queries"));
    return KHP_OK;
}

// ---- ABI 17: queries of the light-path variant (lightpath.h) --------------
// khp_debug_light_paths launches k_light_paths itself on scratch of its own;
// k_dbg_lv_unpack turns its 48-B vertices into the oracle's 10-float records (the
// kernel leaves din / hc of an invalid vertex unwritten: they come back as zeros).
constexpr uint32_t DBG_MAX_VERT = 16;   // khp_bdpt_params.vertices' upper bound

__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_lv_unpack(uint32_t n, const float4* lv, float* out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 a = lv[3 * (size_t)i];
        float* o = out + 10 * (size_t)i;
        const bool ok = a.w != 0.0f;
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 d = ok ? lv[3 * (size_t)i + 1] : z, h = ok ? lv[3 * (size_t)i + 2] : z;
        o[0] = ok ? 1.0f : 0.0f;
        st3(o + 1, ok ? mk(a.x, a.y, a.z) : mk(0.0f, 0.0f, 0.0f));
        st3(o + 4, mk(d.x, d.y, d.z));
        st3(o + 7, mk(h.x, h.y, h.z));
    }
}

// One hit connection per item: trace_closest and surface_at as k_dbg_surface, then
// bd_connection.  recs holds item i's vertex at record DBG_MAX_VERT + i, so that
// bd_connection's v[3 * j] (j < DBG_MAX_VERT) is that record and v stays inside recs.
template <bool TEX>
__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_bdpt_connect(DevScene S, BdptDev bd, uint32_t n, const float* orig,
                                                                const float* dir, const uint32_t* bounce,
                                                                const int32_t* li, const uint32_t* vj,
                                                                const float4* recs, uint8_t* hit, uint8_t* acc,
                                                                float* ro, float* rd, float* tmax, float* cj) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Ray r = make_ray(ld3(orig + 3 * (size_t)i), ld3(dir + 3 * (size_t)i));
        Hit h;
        PrivStack stk;
        TravStats st{0, 0};
        trace_closest<false>(S, r, h, stk, st);
        const v3 zero = mk(0.0f, 0.0f, 0.0f);
        Ray sh;
        sh.o = sh.d = zero;
        float tm = 0.0f;
        v3 col = zero;
        bool ok = false;
        if (h.slot >= 0) {
            ShadeCtx s;
            khp_material mres;
            surface_at<TEX>(S, r, h, s, mres);
            const uint32_t j = vj[i];
            ok = bd_connection(S, bd, recs + 3 * ((size_t)i + DBG_MAX_VERT - j), j, S.lights[li[i]], s, follow(r, h.t),
                               r.d, bounce[i], sh, tm, col);
            if (!ok) {
                sh.o = sh.d = col = zero;
                tm = 0.0f;
            }
        }
        hit[i] = h.slot >= 0 ? 1 : 0;
        acc[i] = ok ? 1 : 0;
        st3(ro + 3 * (size_t)i, sh.o);
        st3(rd + 3 * (size_t)i, sh.d);
        tmax[i] = tm;
        st3(cj + 3 * (size_t)i, col);
    }
}

// One image-plane connection per item: img_sensor and img_connection as k_img_connect.
// recs: DBG_MAX_VERT records of padding, then records j - 1 and j of item i at 2 i and
// 2 i + 1, so that img_connection's lv[3 * (j - 1)] and lv[3 * j] are those and lv stays inside recs.
__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_img_connect(DevScene S, BdptDev bd, uint32_t W, uint32_t H, uint32_t n,
                                                               const float* sensor, const uint32_t* vj,
                                                               const float4* recs, uint8_t* acc, float* dir_out,
                                                               float* t_out, float* cj_out) {
    float a;
    v3 cn;
    img_sensor(S.cam, W, H, a, cn);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t j = vj[i];
        const float4* lv = recs + 3 * (2 * (size_t)i + 1 + DBG_MAX_VERT - j);
        v3 dir = mk(0.0f, 0.0f, 0.0f), cj = dir;
        float t = 0.0f;
        const bool ok = img_connection(bd.img, bd.bias, bd.bounce_bias, lv, j, ld3(sensor + 3 * (size_t)i), a, cn, dir, t, cj);
        if (!ok) {
            dir = cj = mk(0.0f, 0.0f, 0.0f);
            t = 0.0f;
        }
        acc[i] = ok ? 1 : 0;
        st3(dir_out + 3 * (size_t)i, dir);
        t_out[i] = t;
        st3(cj_out + 3 * (size_t)i, cj);
    }
}

static khp_status dbg_bdpt_params(khp_ctx* c) {
    if (c->bd.light_paths < 1 || c->bd.light_paths > 65536) return fail(KHP_EINVAL, "light_paths must be 1..65536");
    if (c->bd.vertices < 1 || c->bd.vertices > DBG_MAX_VERT) return fail(KHP_EINVAL, "vertices must be 1..16");
    return KHP_OK;
}

static BdptDev dbg_bdpt_dev(khp_ctx* c, const float4* lv) {
    return BdptDev{1u, c->bd.light_paths, (uint32_t)c->S.n_lights, c->bd.vertices, c->bd.bias, c->bd.bounce_bias,
                   c->bd.min_pdf, c->bd.image_plane, lv};
}

// 10-float records -> the device's three float4 per vertex
static void dbg_pack_vertex(const float* r, float4* o) {
    o[0] = make_float4(r[1], r[2], r[3], r[0] != 0.0f ? 1.0f : 0.0f);
    o[1] = make_float4(r[4], r[5], r[6], 0.0f);
    o[2] = make_float4(r[7], r[8], r[9], 0.0f);
}

extern "C" khp_status khp_debug_light_paths(khp_ctx* c, uint32_t seed, uint32_t k, float* out) {
    KHPCHK(dbg_enter(c, 1, out != nullptr));
    KHPCHK(dbg_bdpt_params(c));
    if (c->S.n_lights <= 0) return fail(KHP_EINVAL, "the scene has no lights");
    const uint64_t nsub = (uint64_t)c->bd.light_paths * (uint64_t)c->S.n_lights;
    const uint64_t nv = nsub * c->bd.vertices;
    if (nv > DBG_MAX_ITEMS) return fail(KHP_EINVAL, "light_paths x lights x vertices must be at most 2^20");
    DevMem lv, o;
    HIPCHK(lv.ensure(48 * (size_t)nv));
    HIPCHK(o.ensure(40 * (size_t)nv));
    Wave Wv{};   // k_light_paths reads the seed, the sample slots and bd only
    Wv.seed = seed;
    Wv.n_frames = 1;
    Wv.n_samples = 1;
    Wv.sample0 = k;
    Wv.fsample0[0] = k;
    Wv.bd = dbg_bdpt_dev(c, lv.as<float4>());
    hipLaunchKernelGGL(k_light_paths, dim3(((uint32_t)nsub + 63) / 64), dim3(64), 0, c->stream, c->S, Wv);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_dbg_lv_unpack, dim3(dbg_grid((uint32_t)nv)), dim3(DBG_BLOCK), 0, c->stream, (uint32_t)nv,
                       lv.as<float4>(), o.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, o.p, 40 * (size_t)nv, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the light-path query"));
    return KHP_OK;
}

extern "C" khp_status khp_debug_bdpt_connect(khp_ctx* c, uint32_t n, const float* orig, const float* dir,
                                             const uint32_t* bounce, const int32_t* light, const uint32_t* j,
                                             const float* vertex, uint8_t* hit, uint8_t* accepted, float* ray_orig,
                                             float* ray_dir, float* tmax, float* cj) {
    KHPCHK(dbg_enter(c, n, orig && dir && bounce && light && j && vertex && hit && accepted && ray_orig && ray_dir &&
                               tmax && cj));
    KHPCHK(dbg_light_items(c, n, light));
    for (uint32_t i = 0; i < n; ++i) {
        if (j[i] >= DBG_MAX_VERT) return fail(KHP_EINVAL, "item " + std::to_string(i) + ": vertex index must be below 16");
        if (bounce[i] > 4095u) return fail(KHP_EINVAL, "item " + std::to_string(i) + ": bounce must be at most 4095");
    }
    std::vector<float4> recs(3 * ((size_t)n + DBG_MAX_VERT), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t i = 0; i < n; ++i) dbg_pack_vertex(vertex + 10 * (size_t)i, &recs[3 * ((size_t)i + DBG_MAX_VERT)]);
    DevMem o, d, db, dl, dj, dr, oh, oa, oo, od, ot, oc;
    HIPCHK(upload(o, orig, 3 * (size_t)n, c->stream));
    HIPCHK(upload(d, dir, 3 * (size_t)n, c->stream));
    HIPCHK(upload(db, bounce, (size_t)n, c->stream));
    HIPCHK(upload(dl, light, (size_t)n, c->stream));
    HIPCHK(upload(dj, j, (size_t)n, c->stream));
    HIPCHK(upload(dr, recs.data(), recs.size(), c->stream));
    HIPCHK(oh.ensure((size_t)n));
    HIPCHK(oa.ensure((size_t)n));
    HIPCHK(oo.ensure(12 * (size_t)n));
    HIPCHK(od.ensure(12 * (size_t)n));
    HIPCHK(ot.ensure(4 * (size_t)n));
    HIPCHK(oc.ensure(12 * (size_t)n));
    const BdptDev bd = dbg_bdpt_dev(c, nullptr);
    if (c->S.textured)
        hipLaunchKernelGGL(k_dbg_bdpt_connect<true>, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, bd, n,
                           o.as<float>(), d.as<float>(), db.as<uint32_t>(), dl.as<int32_t>(), dj.as<uint32_t>(),
                           dr.as<float4>(), oh.as<uint8_t>(), oa.as<uint8_t>(), oo.as<float>(), od.as<float>(),
                           ot.as<float>(), oc.as<float>());
    else
        hipLaunchKernelGGL(k_dbg_bdpt_connect<false>, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, bd, n,
                           o.as<float>(), d.as<float>(), db.as<uint32_t>(), dl.as<int32_t>(), dj.as<uint32_t>(),
                           dr.as<float4>(), oh.as<uint8_t>(), oa.as<uint8_t>(), oo.as<float>(), od.as<float>(),
                           ot.as<float>(), oc.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hit, oh.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(accepted, oa.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ray_orig, oo.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ray_dir, od.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(tmax, ot.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(cj, oc.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the connection queries"));
    return KHP_OK;
}

extern "C" khp_status khp_debug_img_connect(khp_ctx* c, uint32_t width, uint32_t height, uint32_t n, const float* sensor,
                                            const uint32_t* j, const float* prev, const float* cur, uint8_t* accepted,
                                            float* dir, float* t, float* cj) {
    KHPCHK(dbg_enter(c, n, sensor && j && prev && cur && accepted && dir && t && cj));
    if (width == 0 || height == 0) return fail(KHP_EINVAL, "width and height must be positive");
    if (c->bd.image_plane != 1u && c->bd.image_plane != 2u)
        return fail(KHP_EINVAL, "khp_bdpt_params.image_plane must be 1 or 2");
    for (uint32_t i = 0; i < n; ++i)
        if (j[i] >= DBG_MAX_VERT) return fail(KHP_EINVAL, "item " + std::to_string(i) + ": vertex index must be below 16");
    std::vector<float4> recs(3 * (2 * (size_t)n + DBG_MAX_VERT), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t i = 0; i < n; ++i) {
        dbg_pack_vertex(prev + 10 * (size_t)i, &recs[3 * (2 * (size_t)i + DBG_MAX_VERT)]);
        dbg_pack_vertex(cur + 10 * (size_t)i, &recs[3 * (2 * (size_t)i + 1 + DBG_MAX_VERT)]);
    }
    DevMem ds, dj, dr, oa, od, ot, oc;
    HIPCHK(upload(ds, sensor, 3 * (size_t)n, c->stream));
    HIPCHK(upload(dj, j, (size_t)n, c->stream));
    HIPCHK(upload(dr, recs.data(), recs.size(), c->stream));
    HIPCHK(oa.ensure((size_t)n));
    HIPCHK(od.ensure(12 * (size_t)n));
    HIPCHK(ot.ensure(4 * (size_t)n));
    HIPCHK(oc.ensure(12 * (size_t)n));
    hipLaunchKernelGGL(k_dbg_img_connect, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S,
                       dbg_bdpt_dev(c, nullptr), width, height, n, ds.as<float>(), dj.as<uint32_t>(), dr.as<float4>(),
                       oa.as<uint8_t>(), od.as<float>(), ot.as<float>(), oc.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(accepted, oa.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(dir, od.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(t, ot.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(cj, oc.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the image-plane queries"));
    return KHP_OK;
}

// ---- texture, environment and textured-material queries (after the ABI 15 queries) --------
// tex_color, env_color and the hit's texcoord and resolved material, item by item; the
// same rules as above.  The textures are in HBM only when the scene is textured (a
// textured material parameter or an environment map), so the two that read them refuse
// every other scene before a launch.
__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_tex_color(DevScene S, uint32_t n, const int32_t* tex, const float* xy,
                                                             float* rgba) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 c = tex_color(S, tex[i], xy[2 * (size_t)i], xy[2 * (size_t)i + 1]);
        float* o = rgba + 4 * (size_t)i;
        o[0] = c.x;
        o[1] = c.y;
        o[2] = c.z;
        o[3] = c.w;
    }
}

__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_env_color(DevScene S, uint32_t n, const float* dir, float* rgb) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        st3(rgb + 3 * (size_t)i, env_color(S, ld3(dir + 3 * (size_t)i)));
}

// What k_shade does at a hit of a textured scene: trace_closest, surface_at<true> (which
// resolves the material through textured_material), and hit_texcoord once more with the
// arguments surface_at gave it, for the texcoord itself.  mat: 13 floats per item, diffuse,
// specular, volume and emission rgb, then the roughness.
__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_material(DevScene S, uint32_t n, const float* orig, const float* dir,
                                                            float* t_out, int32_t* obj_out, float* bary, float* tc,
                                                            float* mat) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Ray r = make_ray(ld3(orig + 3 * (size_t)i), ld3(dir + 3 * (size_t)i));
        Hit h;
        PrivStack stk;
        TravStats st{0, 0};
        trace_closest<false>(S, r, h, stk, st);
        int32_t ob = -1;
        float bu = 0.0f, bv = 0.0f, tu = 0.0f, tv = 0.0f;
        khp_material m;
        const v3 zero = mk(0.0f, 0.0f, 0.0f);
        st3(m.diffuse, zero);
        st3(m.specular, zero);
        st3(m.volume, zero);
        st3(m.emission, zero);
        m.roughness = 0.0f;
        if (h.slot >= 0) {
            ShadeCtx s;
            surface_at<true>(S, r, h, s, m);
            const Aux ax = S.aux[h.slot];
            const float4* pr = S.prims + 4 * (size_t)h.slot;
            if (!(ax.flags & 1u)) tri_uv(pr[0], pr[1], pr[2], r, bu, bv);
            hit_texcoord(S, ax, pr, follow(r, h.t), s, bu, bv, tu, tv);
            ob = (int32_t)ax.obj;
        }
        t_out[i] = h.t;
        obj_out[i] = ob;
        bary[2 * (size_t)i] = bu;
        bary[2 * (size_t)i + 1] = bv;
        tc[2 * (size_t)i] = tu;
        tc[2 * (size_t)i + 1] = tv;
        float* o = mat + 13 * (size_t)i;
        st3(o, ld3(m.diffuse));
        st3(o + 3, ld3(m.specular));
        st3(o + 6, ld3(m.volume));
        st3(o + 9, ld3(m.emission));
        o[12] = m.roughness;
    }
}

// khp_debug_camera_rays: camera_path itself, over a chunk description of the items -- item
// i is "pixel" i of an n-pixel list with one sample per pixel, and its sample index goes
// in as the render-ahead offset, so the key is path_key(seed, pixels[i], samples[i]).  LENS
// as the render kernels have it: the instance is chosen by the lens's radius.
template <bool LENS>
__global__ __launch_bounds__(DBG_BLOCK) void k_dbg_camera_rays(DevScene S, Wave Wv, uint32_t n, const uint32_t* samples,
                                                               float* orig, float* dir) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t key_unused;
        const Ray r = camera_path<LENS>(S, Wv, i, key_unused, samples[i]);
        st3(orig + 3 * (size_t)i, r.o);
        st3(dir + 3 * (size_t)i, r.d);
    }
}

extern "C" khp_status khp_debug_camera_rays(khp_ctx* c, uint32_t width, uint32_t seed, uint32_t n,
                                            const uint32_t* pixels, const uint32_t* samples, float* orig, float* dir) {
    if (const char* why = camera_rays_error(nullptr, width, n, pixels, samples, orig, dir))
        return fail(KHP_EINVAL, std::string("khp_debug_camera_rays: ") + why);
    if (!c) return fail(KHP_EINVAL, "khp_debug_camera_rays: ctx is null");
    if (!c->scene_set) return fail(KHP_ENOTREADY, "khp_debug_camera_rays: khp_set_scene first");
    KHPCHK(drain(c));  // complete asynchronous frames first
    HIPCHK(hipSetDevice(c->device));
    DevMem px, sm, oo, od;
    HIPCHK(upload(px, pixels, (size_t)n, c->stream));
    HIPCHK(upload(sm, samples, (size_t)n, c->stream));
    HIPCHK(oo.ensure(12 * (size_t)n));
    HIPCHK(od.ensure(12 * (size_t)n));
    DevScene S{};   // the kernel reads the camera and the lens only
    S.cam = c->hs.cam;
    S.lens = c->S.lens;
    Wave Wv{};
    Wv.pix = px.as<uint32_t>();
    Wv.P = n;
    Wv.W = width;
    Wv.H = 1u;
    Wv.seed = seed;
    Wv.n_samples = 1u;
    Wv.n_frames = 1u;
    if (S.lens.radius > 0.0f)
        hipLaunchKernelGGL(k_dbg_camera_rays<true>, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, S, Wv, n,
                           sm.as<uint32_t>(), oo.as<float>(), od.as<float>());
    else
        hipLaunchKernelGGL(k_dbg_camera_rays<false>, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, S, Wv, n,
                           sm.as<uint32_t>(), oo.as<float>(), od.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(orig, oo.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(dir, od.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the camera ray queries"));
    return KHP_OK;
}

static khp_status dbg_textured(khp_ctx* c, const char* who) {
    if (!c->S.textured)
        return fail(KHP_EINVAL, std::string(who) + ": the scene has no textured material or environment map "
                                                   "(its textures and triangle texcoords are not uploaded)");
    return KHP_OK;
}

extern "C" khp_status khp_debug_tex_color(khp_ctx* c, uint32_t n, const int32_t* tex, const float* xy, float* rgba) {
    KHPCHK(dbg_enter(c, n, tex && xy && rgba));
    KHPCHK(dbg_textured(c, "khp_debug_tex_color"));
    for (uint32_t i = 0; i < n; ++i)
        if (tex[i] < 0 || (size_t)tex[i] >= c->hs.tex.size())
            return fail(KHP_EINVAL, "item " + std::to_string(i) + ": texture index out of range");
    DevMem dt, dx, oc;
    HIPCHK(upload(dt, tex, (size_t)n, c->stream));
    HIPCHK(upload(dx, xy, 2 * (size_t)n, c->stream));
    HIPCHK(oc.ensure(16 * (size_t)n));
    hipLaunchKernelGGL(k_dbg_tex_color, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n, dt.as<int32_t>(),
                       dx.as<float>(), oc.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rgba, oc.p, 16 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the texture queries"));
    return KHP_OK;
}

extern "C" khp_status khp_debug_env_color(khp_ctx* c, uint32_t n, const float* dir, float* rgb) {
    KHPCHK(dbg_enter(c, n, dir && rgb));
    DevMem dd, oc;
    HIPCHK(upload(dd, dir, 3 * (size_t)n, c->stream));
    HIPCHK(oc.ensure(12 * (size_t)n));
    hipLaunchKernelGGL(k_dbg_env_color, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n, dd.as<float>(),
                       oc.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rgb, oc.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the environment queries"));
    return KHP_OK;
}

extern "C" khp_status khp_debug_material(khp_ctx* c, uint32_t n, const float* orig, const float* dir, float* t_out,
                                         int32_t* obj_out, float* bary, float* texcoord, float* diffuse,
                                         float* specular, float* volume, float* emission, float* roughness) {
    KHPCHK(dbg_enter(c, n, orig && dir && t_out && obj_out && bary && texcoord && diffuse && specular && volume &&
                               emission && roughness));
    KHPCHK(dbg_textured(c, "khp_debug_material"));
    DevMem o, d, t, ob, ba, tc, mt;
    HIPCHK(upload(o, orig, 3 * (size_t)n, c->stream));
    HIPCHK(upload(d, dir, 3 * (size_t)n, c->stream));
    HIPCHK(t.ensure(4 * (size_t)n));
    HIPCHK(ob.ensure(4 * (size_t)n));
    HIPCHK(ba.ensure(8 * (size_t)n));
    HIPCHK(tc.ensure(8 * (size_t)n));
    HIPCHK(mt.ensure(52 * (size_t)n));
    hipLaunchKernelGGL(k_dbg_material, dim3(dbg_grid(n)), dim3(DBG_BLOCK), 0, c->stream, c->S, n, o.as<float>(),
                       d.as<float>(), t.as<float>(), ob.as<int32_t>(), ba.as<float>(), tc.as<float>(), mt.as<float>());
    HIPCHK(hipGetLastError());
    std::vector<float> m(13 * (size_t)n);
    HIPCHK(hipMemcpyAsync(t_out, t.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(obj_out, ob.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(bary, ba.p, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(texcoord, tc.p, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(m.data(), mt.p, 52 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the material queries"));
    for (uint32_t i = 0; i < n; ++i) {
        const float* s = &m[13 * (size_t)i];
        memcpy(diffuse + 3 * (size_t)i, s, 12);
        memcpy(specular + 3 * (size_t)i, s + 3, 12);
        memcpy(volume + 3 * (size_t)i, s + 6, 12);
        memcpy(emission + 3 * (size_t)i, s + 9, 12);
        roughness[i] = s[12];
    }
    return KHP_OK;
}
