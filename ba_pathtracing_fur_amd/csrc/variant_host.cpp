// variant_host.cpp -- khp_kernel_variant_host and khp_kernel_variant_table: variant.h's
// selectors and tables, the ones render.hip launches through, answered without a device
// and without a context.
#include "scene.h"
#include "variant.h"

using namespace khp;

static khp_status put(const VariantArgs& a, uint32_t* args, uint32_t* n_args) {
    for (uint32_t i = 0; i < a.n; ++i) args[i] = a.v[i];
    *n_args = a.n;
    return KHP_OK;
}

extern "C" khp_status khp_kernel_variant_host(uint32_t kernel, const khp_variant_facts* q, uint32_t* args,
                                              uint32_t* n_args, uint32_t* grid_kind) {
    if (!q || !args || !n_args) return fail(KHP_EINVAL, "khp_kernel_variant_host: null argument");
    const VariantFacts f{q->textured != 0u, q->fur_only != 0u, q->lobes_on != 0u, q->hair != 0u,
                         q->env != 0u,      q->lens_on != 0u,  q->bd != 0u};
    const bool stats = q->stats != 0u, wide = q->wide != 0u, top = q->top != 0u, has_top = q->has_top != 0u;
    if (grid_kind) *grid_kind = 0u;
    switch (kernel) {
    case KHP_KERNEL_PATH: return put(select_path(f, wide, q->ahead != 0u, q->queue_start != 0u).args(), args, n_args);
    case KHP_KERNEL_SHADE: {
        const ShadeVariant v = select_shade(f, q->bounce, q->cam0 != 0u);
        if (grid_kind) *grid_kind = v.bd ? 1u : 0u;
        return put(v.args(), args, n_args);
    }
    case KHP_KERNEL_EXTEND: return put(select_extend(f, stats, q->cam != 0u, wide, top, has_top).args(), args, n_args);
    case KHP_KERNEL_SHADOW: return put(select_shadow(stats, wide, top, has_top).args(), args, n_args);
    case KHP_KERNEL_AOV_TRACE: return put(select_aov(f).args(), args, n_args);
    case KHP_KERNEL_GENERATE: return put(select_generate(f).args(), args, n_args);
    case KHP_KERNEL_SHADOW_FINISH: return put(select_shadow_finish(f.bd).args(), args, n_args);
    }
    return fail(KHP_EINVAL, "khp_kernel_variant_host: unknown kernel family");
}

template <class V, size_t N>
static khp_status row(const std::array<V, N>& table, uint32_t index, uint32_t* args, uint32_t* n_args) {
    if (index >= N) return fail(KHP_EINVAL, "khp_kernel_variant_table: index past the table's end");
    return put(table[index].args(), args, n_args);
}

extern "C" khp_status khp_kernel_variant_table(uint32_t kernel, uint32_t index, uint32_t* args, uint32_t* n_args) {
    if (!args || !n_args) return fail(KHP_EINVAL, "khp_kernel_variant_table: null argument");
    switch (kernel) {
    case KHP_KERNEL_PATH: return row(PATH_TABLE, index, args, n_args);
    case KHP_KERNEL_SHADE: return row(SHADE_TABLE, index, args, n_args);
    case KHP_KERNEL_EXTEND: return row(EXTEND_TABLE, index, args, n_args);
    case KHP_KERNEL_SHADOW: return row(SHADOW_TABLE, index, args, n_args);
    case KHP_KERNEL_AOV_TRACE: return row(AOV_TABLE, index, args, n_args);
    case KHP_KERNEL_GENERATE: return row(GENERATE_TABLE, index, args, n_args);
    case KHP_KERNEL_SHADOW_FINISH: return row(SHADOW_FINISH_TABLE, index, args, n_args);
    }
    return fail(KHP_EINVAL, "khp_kernel_variant_table: unknown kernel family");
}
