// kmath_host.cpp -- khp_kmath_host: kmath.h as the host compiler builds it, op by op
// over a batch of raw items (kmath_ops.h).  The plain loop; it needs no device and no
// context.
#include "kmath_ops.h"
#include "scene.h"

extern "C" khp_status khp_kmath_host(uint32_t op, uint32_t n, const uint64_t* in, uint64_t* out) {
    using namespace khp;
    if (const char* why = kmath_args_error(op, n, in, out)) return fail(KHP_EINVAL, std::string("khp_kmath_host: ") + why);
    for (uint32_t i = 0; i < n; ++i) kmath_apply(op, in + KMATH_WORDS * (size_t)i, out + KMATH_WORDS * (size_t)i);
    return KHP_OK;
}
