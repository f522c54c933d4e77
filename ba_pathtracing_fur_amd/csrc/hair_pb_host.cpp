// hair_pb_host.cpp -- khp_hair_material, khp_hair_eval_host and khp_hair_sample_host: the
// host side of BSDF kind 11.  The functions are hair_pb.h's, the ones the gfx950 kernels
// compile too; these are plain loops over them, a reference that needs no device and no
// context.
#include "hair_pb.h"
#include "scene.h"

extern "C" khp_status khp_hair_material(const float color[3], float beta_m, float beta_n, float alpha_deg, float ior,
                                        khp_material* out) {
    using namespace khp;
    if (!color || !out) return fail(KHP_EINVAL, "khp_hair_material: null argument");
    for (int c = 0; c < 3; ++c)
        if (!(color[c] > 0.0f && color[c] <= 1.0f)) return fail(KHP_EINVAL, "khp_hair_material: color must be in (0, 1]");
    khp_material m{};
    m.bsdf = KHP_BSDF_CHIANG_HAIR;
    m.shader = KHP_SHADER_SIMPLE;
    m.roughness = beta_m;
    m.specular[0] = beta_n;
    m.specular[1] = alpha_deg;
    m.specular[2] = 0.0f;
    m.ior = ior;
    if (const char* why = hair_material_error(m)) return fail(KHP_EINVAL, std::string("khp_hair_material: ") + why);
    // Chiang's colour map: the absorption that gives a thick groom of these fibres the colour
    const float b = beta_n, b2 = b * b, b3 = b2 * b, b4 = b3 * b, b5 = b4 * b;
    const float d = ((((5.969f - 0.215f * b) + 2.532f * b2) - 10.73f * b3) + 5.574f * b4) + 0.245f * b5;
    for (int c = 0; c < 3; ++c) {
        m.diffuse[c] = color[c];
        const float q = k_logf_d(color[c]) / d;
        m.volume[c] = q * q;
    }
    *out = m;
    return KHP_OK;
}

namespace khp {
static const char* hair_items_error(uint32_t n, const khp_material* mats, bool ptrs_ok, std::string& msg) {
    if (!ptrs_ok) return "null argument";
    if (n == 0u || n > (1u << 20)) return "n must be in [1, 2^20]";
    for (uint32_t i = 0; i < n; ++i) {
        if (mats[i].bsdf != KHP_BSDF_CHIANG_HAIR) {
            msg = "item " + std::to_string(i) + ": material is not KHP_BSDF_CHIANG_HAIR";
            return msg.c_str();
        }
    }
    return nullptr;
}
}  // namespace khp

extern "C" khp_status khp_hair_eval_host(uint32_t n, const khp_material* materials, const float* uvw,
                                         const float* normal, const float* wo, const float* wi, float* f) {
    using namespace khp;
    std::string msg;
    if (const char* why = hair_items_error(n, materials, materials && uvw && normal && wo && wi && f, msg))
        return fail(KHP_EINVAL, std::string("khp_hair_eval_host: ") + why);
    for (uint32_t i = 0; i < n; ++i) {
        const float* fr = uvw + 9 * (size_t)i;
        const v3 r = hair_pb_eval(materials[i], ld3(fr), ld3(fr + 3), ld3(fr + 6), ld3(normal + 3 * (size_t)i),
                                  ld3(wo + 3 * (size_t)i), ld3(wi + 3 * (size_t)i));
        f[3 * (size_t)i] = r.x; f[3 * (size_t)i + 1] = r.y; f[3 * (size_t)i + 2] = r.z;
    }
    return KHP_OK;
}

extern "C" khp_status khp_hair_sample_host(uint32_t n, const khp_material* materials, const float* uvw,
                                           const float* normal, const float* wo, const float* draws, float* out_dir,
                                           float* pdf, float* f, int32_t* valid) {
    using namespace khp;
    std::string msg;
    if (const char* why = hair_items_error(n, materials, materials && uvw && normal && wo && draws && out_dir && pdf &&
                                                             f && valid, msg))
        return fail(KHP_EINVAL, std::string("khp_hair_sample_host: ") + why);
    for (uint32_t i = 0; i < n; ++i) {
        const float* fr = uvw + 9 * (size_t)i;
        const float* u = draws + 4 * (size_t)i;
        v3 o;
        float pd;
        bool ok;
        const v3 r = hair_pb_sample(materials[i], ld3(fr), ld3(fr + 3), ld3(fr + 6), ld3(normal + 3 * (size_t)i),
                                    ld3(wo + 3 * (size_t)i), u[0], u[1], u[2], u[3], o, pd, ok);
        out_dir[3 * (size_t)i] = o.x; out_dir[3 * (size_t)i + 1] = o.y; out_dir[3 * (size_t)i + 2] = o.z;
        f[3 * (size_t)i] = r.x; f[3 * (size_t)i + 1] = r.y; f[3 * (size_t)i + 2] = r.z;
        pdf[i] = pd;
        valid[i] = ok ? 1 : 0;
    }
    return KHP_OK;
}
