// env_light.h -- khp_set_env_light: a latitude-longitude map of float32 radiance as a light
// that next-event rays are aimed at.  The sampling table, the sampler and the evaluation
// are plain functions compiled by g++ (env_light_host.cpp: the khp_env_light_*_host
// entries) and by hipcc (env_light_dev.h builds the table, render.hip's shade_core samples
// and evaluates), both with -ffp-contract=off: the same bits on host and device.  Every
// float step is one float32 operation in the order written; the table is integers, so any
// order of summation builds the same one.
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/kirk_hip.h"
#include "kmath.h"

namespace khp {

constexpr uint32_t ENV_W_MAX = 4096u, ENV_H_MAX = 2048u;
constexpr float ENV_WEIGHT_SCALE = 524288.0f;          // 2^19: a row of 4096 weights sums below 2^32
constexpr float ENV_ROTATION_MAX = 8192.0f;            // |rotation| beyond this is refused (k_sinf's range)
constexpr float ENV_TWO_PI = 6.283185482025146484375f;         // 2 pi rounded to float32 (0x40C90FDB)
constexpr float ENV_TWO_PI_SQ = 19.739208221435546875f;        // 2 pi^2 rounded to float32
constexpr float ENV_BELOW_ONE = 0.999999940395355224609375f;   // 1 - 2^-24
// The bit a path's flags (TFq[].w) carry away from a hit that aimed, or could have aimed, a
// next-event ray at the map: an escaping ray of such a path does not add the map again.
enum : int { F_ENV_NEE = 32 };

// The map, its parameters and its table as the functions below read them (host or device
// pointers).  dth and dph are pi / H and 2 pi / W as float32 quotients.
struct EnvLight {
    uint32_t W, H;
    uint32_t nee;
    float scale, rotation, select;
    float dth, dph;
    const float* rgb;           // [H][W][3]
    const uint32_t* weight;     // [H][W]
    const uint32_t* row_cdf;    // [H][W + 1]: exclusive prefix of a row, the row's sum last
    const uint64_t* marginal;   // [H + 1]: exclusive prefix of the row sums, the total last
};

// Why khp_set_env_light refuses *e's parameters (the texels are checked apart), or null.
inline const char* env_light_param_error(const khp_env_light* e) {
    if (!e) return "null argument";
    if (e->width < 1u || e->width > ENV_W_MAX) return "width must be 1..4096";
    if (e->height < 1u || e->height > ENV_H_MAX) return "height must be 1..2048";
    if (e->flags & ~(uint32_t)KHP_ENV_LIGHT_DEVICE) return "unknown flags";
    if (e->nee > 1u) return "nee must be 0 or 1";
    if (!(e->scale > 0.0f) || e->scale == k_inf()) return "scale must be finite and > 0";
    if (!(k_fabs(e->rotation) <= ENV_ROTATION_MAX)) return "rotation must be finite, at most 8192 radians either way";
    if (!(e->select > 0.0f) || !(e->select <= 1.0f)) return "select must be in (0, 1]";
    if (e->reserved != 0u) return "reserved must be 0";
    if (!e->rgb) return "rgb is null";
    return nullptr;
}

KHD bool env_texel_bad(float r, float g, float b) {
    // finite and >= 0: a NaN fails the first comparison, an infinity the second
    return !(r >= 0.0f && g >= 0.0f && b >= 0.0f) || r == k_inf() || g == k_inf() || b == k_inf();
}

KHD float env_dth(uint32_t H) { return PIF / (float)H; }
KHD float env_dph(uint32_t W) { return ENV_TWO_PI / (float)W; }

// y s_j of texel (i, j): the luminance times the sine of the row's mid latitude.
KHD float env_row_sin(uint32_t j, float dth) { return k_sinf(((float)j + 0.5f) * dth); }
KHD float env_importance(float r, float g, float b, float sj) {
    const float y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    return y * sj;
}
// The integer weight of a texel whose importance is p, m the map's largest.
KHD uint32_t env_weight(float p, float m) {
    if (!(p > 0.0f)) return 0u;
    const uint32_t q = (uint32_t)((p / m) * ENV_WEIGHT_SCALE);
    return q < 1u ? 1u : q;
}

KHD uint32_t env_draw_bits(float u) {
    const float s = u * 16777216.0f;
    if (!(s > 0.0f)) return 0u;
    if (s >= 16777215.0f) return 16777215u;
    return (uint32_t)s;
}
// floor(U t / 2^24) for U < 2^24 and any 64-bit t
KHD uint64_t env_scale_u24(uint32_t U, uint64_t t) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi((uint64_t)U << 40, t);
#else
    return (uint64_t)(((unsigned __int128)((uint64_t)U << 40) * (unsigned __int128)t) >> 64);
#endif
}

// Nearest-texel radiance (times scale) and solid-angle density of direction d.
// texel: the index j * W + i the direction fell in.  A direction that is not a direction
// (zero, NaN) has radiance 0 and density 0.
KHD void env_light_eval(const EnvLight& E, v3 d, v3& radiance, float& pdf, uint32_t& texel) {
    radiance = mk(0.0f, 0.0f, 0.0f);
    pdf = 0.0f;
    texel = 0u;
    const v3 n = normalize(d);
    if (!(n.x == n.x) || !(n.y == n.y) || !(n.z == n.z)) return;
    const float ny = gclamp(n.y, -1.0f, 1.0f);
    const float th = k_asinf(ny) + PIO2F;           // from the -y pole
    const float ph = k_atan2f(n.z, n.x) - E.rotation;
    const float fj = th / E.dth;
    int j = (int)fj;
    j = j < 0 ? 0 : (j > (int)E.H - 1 ? (int)E.H - 1 : j);
    const float t0 = ph / ENV_TWO_PI;
    const float t = t0 - floorf(t0);
    const float fi = t * (float)E.W;
    int i = (int)fi;
    i = i < 0 ? 0 : (i > (int)E.W - 1 ? (int)E.W - 1 : i);
    texel = (uint32_t)j * E.W + (uint32_t)i;
    const float* p = E.rgb + 3 * (size_t)texel;
    radiance = mk(p[0] * E.scale, p[1] * E.scale, p[2] * E.scale);
    // sin(theta) as the length of the horizontal part: sqrt(1 - n.y^2) loses it near the poles
    const float root = k_sqrt(n.x * n.x + n.z * n.z);
    if (root == 0.0f) return;
    const float share = (float)E.weight[texel] / (float)E.marginal[E.H];
    pdf = (share * (float)(E.W * E.H)) / (ENV_TWO_PI_SQ * root);
}

// A direction drawn from the table by (u0, u1), with eval's radiance and density of that
// direction.  texel: the one the integer walk chose.  valid: the density is > 0.
KHD void env_light_sample(const EnvLight& E, float u0, float u1, v3& d, v3& radiance, float& pdf, uint32_t& texel,
                          bool& valid) {
    const uint32_t U0 = env_draw_bits(u0), U1 = env_draw_bits(u1);
    const uint64_t X = env_scale_u24(U0, E.marginal[E.H]);
    uint32_t lo = 0u, hi = E.H;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (E.marginal[mid] <= X) lo = mid; else hi = mid;
    }
    const uint32_t j = lo;
    const uint32_t* row = E.row_cdf + (size_t)j * (E.W + 1u);
    const uint32_t rowsum = row[E.W];
    const uint32_t Y = (uint32_t)(((uint64_t)U1 * (uint64_t)rowsum) >> 24);
    lo = 0u;
    hi = E.W;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (row[mid] <= Y) lo = mid; else hi = mid;
    }
    const uint32_t i = lo;
    texel = j * E.W + i;
    const float fy = gmin(((float)(uint32_t)(X - E.marginal[j]) + 0.5f) / (float)rowsum, ENV_BELOW_ONE);
    const float fx = gmin(((float)(Y - row[i]) + 0.5f) / (float)(row[i + 1u] - row[i]), ENV_BELOW_ONE);
    const float th = ((float)j + fy) * E.dth;
    const float ph = ((float)i + fx) * E.dph + E.rotation;
    const float st = k_sinf(th), ct = k_cosf(th);
    d = mk(st * k_cosf(ph), -ct, st * k_sinf(ph));
    uint32_t et;
    env_light_eval(E, d, radiance, pdf, et);
    valid = pdf > 0.0f;
}

// The host loops that define the table (env_light_host.cpp); the device builds the same
// words in parallel (env_light_dev.h).  False: the map is black.
bool env_light_tables(const float* rgb, uint32_t W, uint32_t H, uint32_t* weight, uint32_t* row_cdf,
                      uint64_t* marginal);
// The first bad texel of a host map as text, or an empty string.
std::string env_light_texel_error(const float* rgb, uint32_t W, uint32_t H);

}  // namespace khp
