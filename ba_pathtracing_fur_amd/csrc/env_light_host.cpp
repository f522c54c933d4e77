// env_light_host.cpp -- khp_env_light_defaults and the three khp_env_light_*_host entries:
// the host side of the environment light.  The functions are env_light.h's, the ones the
// gfx950 kernels compile too; these are plain loops over them, a reference that needs no
// device and no context.
#include "env_light.h"
#include "scene.h"

#include <algorithm>
#include <vector>

extern "C" void khp_env_light_defaults(khp_env_light* out) {
    if (!out) return;
    *out = khp_env_light{};
    out->nee = 1u;
    out->scale = 1.0f;
    out->rotation = 0.0f;
    out->select = 0.5f;
}

namespace khp {

std::string env_light_texel_error(const float* rgb, uint32_t W, uint32_t H) {
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            const float* p = rgb + 3 * ((size_t)j * W + i);
            if (env_texel_bad(p[0], p[1], p[2]))
                return "texel (" + std::to_string(i) + ", " + std::to_string(j) + ") is negative or not finite";
        }
    return std::string();
}

bool env_light_tables(const float* rgb, uint32_t W, uint32_t H, uint32_t* weight, uint32_t* row_cdf,
                      uint64_t* marginal) {
    const float dth = env_dth(H);
    float m = 0.0f;
    for (uint32_t j = 0; j < H; ++j) {
        const float sj = env_row_sin(j, dth);
        for (uint32_t i = 0; i < W; ++i) {
            const float* p = rgb + 3 * ((size_t)j * W + i);
            m = gmax(m, env_importance(p[0], p[1], p[2], sj));
        }
    }
    if (!(m > 0.0f)) return false;
    uint64_t total = 0;
    for (uint32_t j = 0; j < H; ++j) {
        const float sj = env_row_sin(j, dth);
        uint32_t sum = 0;
        uint32_t* row = row_cdf + (size_t)j * (W + 1u);
        for (uint32_t i = 0; i < W; ++i) {
            const float* p = rgb + 3 * ((size_t)j * W + i);
            const uint32_t w = env_weight(env_importance(p[0], p[1], p[2], sj), m);
            weight[(size_t)j * W + i] = w;
            row[i] = sum;
            sum += w;
        }
        row[W] = sum;
        marginal[j] = total;
        total += sum;
    }
    marginal[H] = total;
    return true;
}

namespace {
// A host map's light with its table, as the entries below need it.
struct HostEnvLight {
    std::vector<uint32_t> weight, row_cdf;
    std::vector<uint64_t> marginal;
    EnvLight E{};
};
khp_status host_env_light(const char* who, const khp_env_light* l, HostEnvLight& h) {
    if (const char* why = env_light_param_error(l)) return fail(KHP_EINVAL, std::string(who) + ": " + why);
    if (l->flags & KHP_ENV_LIGHT_DEVICE) return fail(KHP_EINVAL, std::string(who) + ": a host entry takes a host map");
    const std::string bad = env_light_texel_error(l->rgb, l->width, l->height);
    if (!bad.empty()) return fail(KHP_EINVAL, std::string(who) + ": " + bad);
    const uint32_t W = l->width, H = l->height;
    h.weight.resize((size_t)W * H);
    h.row_cdf.resize((size_t)(W + 1u) * H);
    h.marginal.resize((size_t)H + 1u);
    if (!env_light_tables(l->rgb, W, H, h.weight.data(), h.row_cdf.data(), h.marginal.data()))
        return fail(KHP_EINVAL, std::string(who) + ": the map is black");
    h.E.W = W;
    h.E.H = H;
    h.E.nee = l->nee;
    h.E.scale = l->scale;
    h.E.rotation = l->rotation;
    h.E.select = l->select;
    h.E.dth = env_dth(H);
    h.E.dph = env_dph(W);
    h.E.rgb = l->rgb;
    h.E.weight = h.weight.data();
    h.E.row_cdf = h.row_cdf.data();
    h.E.marginal = h.marginal.data();
    return KHP_OK;
}
}  // namespace
}  // namespace khp

extern "C" khp_status khp_env_light_tables_host(const khp_env_light* light, uint32_t* weight, uint32_t* row_cdf,
                                                uint64_t* marginal) {
    using namespace khp;
    if (!weight || !row_cdf || !marginal) return fail(KHP_EINVAL, "khp_env_light_tables_host: null argument");
    HostEnvLight h;
    const khp_status st = host_env_light("khp_env_light_tables_host", light, h);
    if (st != KHP_OK) return st;
    std::copy(h.weight.begin(), h.weight.end(), weight);
    std::copy(h.row_cdf.begin(), h.row_cdf.end(), row_cdf);
    std::copy(h.marginal.begin(), h.marginal.end(), marginal);
    return KHP_OK;
}

extern "C" khp_status khp_env_light_sample_host(const khp_env_light* light, uint32_t n, const float* draws, float* dir,
                                                float* pdf, float* radiance, int32_t* valid) {
    using namespace khp;
    if (!draws || !dir || !pdf || !radiance || !valid)
        return fail(KHP_EINVAL, "khp_env_light_sample_host: null argument");
    if (n == 0u || n > (1u << 20)) return fail(KHP_EINVAL, "khp_env_light_sample_host: n must be in [1, 2^20]");
    HostEnvLight h;
    const khp_status st = host_env_light("khp_env_light_sample_host", light, h);
    if (st != KHP_OK) return st;
    for (uint32_t k = 0; k < n; ++k) {
        v3 d, L;
        float p;
        uint32_t texel;
        bool ok;
        env_light_sample(h.E, draws[2 * (size_t)k], draws[2 * (size_t)k + 1], d, L, p, texel, ok);
        dir[3 * (size_t)k] = d.x; dir[3 * (size_t)k + 1] = d.y; dir[3 * (size_t)k + 2] = d.z;
        radiance[3 * (size_t)k] = L.x; radiance[3 * (size_t)k + 1] = L.y; radiance[3 * (size_t)k + 2] = L.z;
        pdf[k] = p;
        valid[k] = ok ? 1 : 0;
    }
    return KHP_OK;
}

extern "C" khp_status khp_env_light_eval_host(const khp_env_light* light, uint32_t n, const float* dir,
                                              float* radiance, float* pdf) {
    using namespace khp;
    if (!dir || !radiance || !pdf) return fail(KHP_EINVAL, "khp_env_light_eval_host: null argument");
    if (n == 0u || n > (1u << 20)) return fail(KHP_EINVAL, "khp_env_light_eval_host: n must be in [1, 2^20]");
    HostEnvLight h;
    const khp_status st = host_env_light("khp_env_light_eval_host", light, h);
    if (st != KHP_OK) return st;
    for (uint32_t k = 0; k < n; ++k) {
        v3 L;
        float p;
        uint32_t texel;
        env_light_eval(h.E, ld3(dir + 3 * (size_t)k), L, p, texel);
        radiance[3 * (size_t)k] = L.x; radiance[3 * (size_t)k + 1] = L.y; radiance[3 * (size_t)k + 2] = L.z;
        pdf[k] = p;
    }
    return KHP_OK;
}
