// variant.h -- which compile-time instance of a render kernel a launch takes.
// Plain C++17, no HIP: render.hip launches through these tables, variant_host.cpp answers
// the same questions without a device.  Per kernel family: a descriptor (the template
// arguments by name, in declaration order), a selector from the facts of a batch and the
// inputs of one launch to a descriptor, and the table of the instances that are compiled.
// A descriptor the table does not hold is refused at the launch; nothing else is compiled.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <array>

#include "../../include/kirk_hip.h"

namespace khp {

// BSDF kind sets k_shade and k_path are instantiated for (bit k = khp_bsdf_kind k): every
// kind, or the fur scenes' (Lambert reflection + Marschner hair: configs 1-3 and the metric
// row), where the other kinds' code and registers are compiled out.
constexpr uint32_t KINDS_ALL = 0x7FFu;   // KIRK's eleven kinds
constexpr uint32_t KINDS_FUR = (1u << KHP_BSDF_LAMBERTIAN_REFLECTION) | (1u << KHP_BSDF_MARSCHNER_HAIR);
// Scenes with a kind-11 material (hair_pb.h) take one covering set: the eleven and ChiangHairBSDF.
constexpr uint32_t KINDS_ALL_HAIR = (1u << KHP_BSDF_COUNT) - 1u;
constexpr uint32_t KINDS_FUR_HAIR = (1u << KHP_BSDF_LAMBERTIAN_REFLECTION) | (1u << KHP_BSDF_CHIANG_HAIR);
static_assert(KINDS_ALL_HAIR == 0xFFFu, "the covering set of scenes with kind 11");
// A spare bit of the sets above: the instance traces Marschner's TT and TRT paths
// (khp_set_hair_lobes).  The all-ones default of KINDS predates the bit and means every
// BSDF kind with the R lobe only: k_shade's default, a different instance from KINDS_ALL.
constexpr uint32_t KINDS_LOBES = 1u << 31;
constexpr uint32_t KINDS_DEFAULT = 0xFFFFFFFFu;

// A descriptor as its template arguments in declaration order: what two descriptors are
// compared by, and what khp_kernel_variant_host returns.
struct VariantArgs {
    uint32_t n;
    uint32_t v[7];
};
constexpr bool operator==(const VariantArgs& a, const VariantArgs& b) {
    bool same = a.n == b.n;
    for (uint32_t i = 0; same && i < a.n; ++i) same = a.v[i] == b.v[i];
    return same;
}

struct ShadeVariant {
    bool tex, bd;
    uint32_t kinds;
    bool lens, env;
    constexpr VariantArgs args() const { return {5, {tex, bd, kinds, lens, env}}; }
};
struct PathVariant {
    bool tex, wide;
    uint32_t kinds;
    bool ra, qs, lens, env;
    constexpr VariantArgs args() const { return {7, {tex, wide, kinds, ra, qs, lens, env}}; }
};
struct ExtendVariant {
    bool stats, cam, wide, top, lens;
    constexpr VariantArgs args() const { return {5, {stats, cam, wide, top, lens}}; }
};
struct ShadowVariant {
    bool stats, wide, top;
    constexpr VariantArgs args() const { return {3, {stats, wide, top}}; }
};
struct AovVariant {
    bool tex, lens;
    constexpr VariantArgs args() const { return {2, {tex, lens}}; }
};
struct GenerateVariant {
    bool lens;
    constexpr VariantArgs args() const { return {1, {lens}}; }
};
struct ShadowFinishVariant {
    bool bd;
    constexpr VariantArgs args() const { return {1, {bd}}; }
};

// What the choice is made from, beside the inputs of the one launch: the scene has textures;
// only KINDS_FUR's kinds; khp_set_hair_lobes other than R; a ChiangHairBSDF material;
// khp_set_env_light; khp_set_lens with a radius; the light-path variant runs.
struct VariantFacts {
    bool textured, fur_only, lobes_on, hair, env, lens_on, bd;
};

// The kind set of a k_shade or k_path instance without the environment light.  `every`:
// how the family names "every kind" (KINDS_DEFAULT for k_shade, KINDS_ALL for k_path).
constexpr uint32_t select_kinds(const VariantFacts& f, bool bd, uint32_t every) {
    if (f.hair) return KINDS_ALL_HAIR;   // ChiangHairBSDF compiled in
    if (f.lobes_on) return ((!f.textured && f.fur_only) ? KINDS_FUR : KINDS_ALL) | KINDS_LOBES;   // TT / TRT compiled in
    if (f.textured || bd) return every;
    return f.fur_only ? KINDS_FUR : every;   // fur scenes: the other BSDF kinds compiled out
}

// k_shade of bounce `bounce`.  The lens twin runs for the one launch that recomputes camera rays.
// The environment light, ChiangHairBSDF and the lobes have no light-path instance (their setters
// refuse the combination); they take precedence here.  The grid: grid_shade_bd where .bd, else grid_shade.
constexpr ShadeVariant select_shade(const VariantFacts& f, uint32_t bounce, bool cam0) {
    const bool lens = !f.bd && bounce == 0u && cam0 && f.lens_on;
    if (f.env) return {f.textured, false, KINDS_ALL_HAIR, lens, true};
    const bool bd = f.bd && !f.hair && !f.lobes_on;
    return {f.textured, bd, select_kinds(f, bd, KINDS_DEFAULT), lens, false};
}

// k_path.  A queue start (hybrid batches) makes no camera ray and renders nothing ahead.
constexpr PathVariant select_path(const VariantFacts& f, bool wide, bool ahead, bool queue_start) {
    return {f.textured, wide, f.env ? KINDS_ALL_HAIR : select_kinds(f, false, KINDS_ALL),
            !queue_start && ahead, queue_start, !queue_start && f.lens_on, f.env};
}

// k_extend and k_shadow.  top: khp_ctx_params.lds_nodes asks for the top records in LDS; has_top:
// the tree has them.  The LDS bytes follow the descriptor: the camera's or the plain loop's, plus
// the top records' where .top.
constexpr ExtendVariant select_extend(const VariantFacts& f, bool stats, bool cam, bool wide, bool top, bool has_top) {
    const bool lens = cam && f.lens_on;
    if (top && !stats && !wide && has_top) return {false, cam, false, true, lens};
    return {stats, cam, wide, false, lens};
}
constexpr ShadowVariant select_shadow(bool stats, bool wide, bool top, bool has_top) {
    if (top && !stats && !wide && has_top) return {false, false, true};
    return {stats, wide, false};
}
constexpr AovVariant select_aov(const VariantFacts& f) { return {f.textured, f.lens_on}; }
constexpr GenerateVariant select_generate(const VariantFacts& f) { return {f.lens_on}; }
constexpr ShadowFinishVariant select_shadow_finish(bool bd) { return {bd}; }

// ---- the compiled instances: 22 + 100 + 15 + 5 + 4 + 2 + 2 ----------------------------------
// A builder that fills other than its N rows does not compile (the throw is then evaluated).
template <class V, size_t N>
constexpr std::array<V, N> filled(const std::array<V, N>& t, size_t n) {
    return n == N ? t : throw "variant.h: a table's row count";
}
constexpr bool BOTH[2] = {false, true};

// 10 (tex, bd, kinds) triples, a lens twin of each but the light-path ones; tex x lens with the environment light.
constexpr std::array<ShadeVariant, 22> shade_table() {
    constexpr ShadeVariant base[10] = {
        {true, false, KINDS_ALL_HAIR},           {false, false, KINDS_ALL_HAIR},
        {true, false, KINDS_ALL | KINDS_LOBES},  {false, false, KINDS_FUR | KINDS_LOBES},
        {false, false, KINDS_ALL | KINDS_LOBES}, {true, true, KINDS_DEFAULT},
        {true, false, KINDS_DEFAULT},            {false, true, KINDS_DEFAULT},
        {false, false, KINDS_FUR},               {false, false, KINDS_DEFAULT}};
    std::array<ShadeVariant, 22> t{};
    size_t n = 0;
    for (const ShadeVariant& b : base)
        for (bool lens : BOTH)
            if (!(lens && b.bd)) t[n++] = {b.tex, b.bd, b.kinds, lens, false};
    for (bool tex : BOTH)
        for (bool lens : BOTH) t[n++] = {tex, false, KINDS_ALL_HAIR, lens, true};
    return filled(t, n);
}
// 8 (tex, kinds) pairs x wide x 5 (ra, qs, lens) triples; tex x wide x the 5 with the environment light.
constexpr std::array<PathVariant, 100> path_table() {
    constexpr PathVariant base[8] = {
        {true, false, KINDS_ALL_HAIR},           {false, false, KINDS_ALL_HAIR},
        {true, false, KINDS_ALL | KINDS_LOBES},  {false, false, KINDS_FUR | KINDS_LOBES},
        {false, false, KINDS_ALL | KINDS_LOBES}, {true, false, KINDS_ALL},
        {false, false, KINDS_FUR},               {false, false, KINDS_ALL}};
    constexpr bool rql[5][3] = {{false, true, false}, {false, false, false}, {true, false, false},
                                {false, false, true}, {true, false, true}};
    std::array<PathVariant, 100> t{};
    size_t n = 0;
    for (const PathVariant& b : base)
        for (bool wide : BOTH)
            for (const auto& r : rql) t[n++] = {b.tex, wide, b.kinds, r[0], r[1], r[2], false};
    for (bool tex : BOTH)
        for (bool wide : BOTH)
            for (const auto& r : rql) t[n++] = {tex, wide, KINDS_ALL_HAIR, r[0], r[1], r[2], true};
    return filled(t, n);
}
// stats x cam x wide, a lens twin of each cam one; the top records in LDS: the plain loop, the camera's, its lens twin.
constexpr std::array<ExtendVariant, 15> extend_table() {
    std::array<ExtendVariant, 15> t{};
    size_t n = 0;
    for (bool stats : BOTH)
        for (bool cam : BOTH)
            for (bool wide : BOTH)
                for (bool lens : BOTH)
                    if (!(lens && !cam)) t[n++] = {stats, cam, wide, false, lens};
    t[n++] = {false, false, false, true, false};
    t[n++] = {false, true, false, true, false};
    t[n++] = {false, true, false, true, true};
    return filled(t, n);
}
// stats x wide; the top records in LDS.
constexpr std::array<ShadowVariant, 5> shadow_table() {
    std::array<ShadowVariant, 5> t{};
    size_t n = 0;
    for (bool stats : BOTH)
        for (bool wide : BOTH) t[n++] = {stats, wide, false};
    t[n++] = {false, false, true};
    return filled(t, n);
}
constexpr std::array<ShadeVariant, 22> SHADE_TABLE = shade_table();
constexpr std::array<PathVariant, 100> PATH_TABLE = path_table();
constexpr std::array<ExtendVariant, 15> EXTEND_TABLE = extend_table();
constexpr std::array<ShadowVariant, 5> SHADOW_TABLE = shadow_table();
constexpr std::array<AovVariant, 4> AOV_TABLE = {{{false, false}, {false, true}, {true, false}, {true, true}}};
constexpr std::array<GenerateVariant, 2> GENERATE_TABLE = {{{false}, {true}}};
constexpr std::array<ShadowFinishVariant, 2> SHADOW_FINISH_TABLE = {{{false}, {true}}};

}  // namespace khp
