// env_light_dev.h -- khp_set_env_light on the device (included by render.hip): the kernels
// that check a device map and build the sampling table of env_light.h, the context's
// entry points and the two khp_debug_env_light* queries.  The table is integers, so the
// parallel scans here give khp_env_light_tables_host's words.
#pragma once

constexpr uint32_t ENV_BLOCK = 256;
constexpr uint32_t ENV_NO_TEXEL = 0xFFFFFFFFu;

// The build's two scalars: the bit pattern of m = max importance (non-negative floats order
// as their bits do) and the first bad texel of the map.
struct EnvBuildFlags {
    uint32_t m_bits;
    uint32_t bad_texel;
};

// One launch: every texel's importance, a wave max by cross-lane exchange, a block max through
// LDS, one atomic per block; a texel that is negative or not finite lowers bad_texel to its index.
__global__ __launch_bounds__(ENV_BLOCK) void k_env_max(const float* __restrict__ rgb, uint32_t W, uint32_t H, float dth,
                                                       EnvBuildFlags* fl) {
    __shared__ float wmax[ENV_BLOCK / 64];
    const uint32_t n = W * H;
    float m = 0.0f;
    uint32_t bad = ENV_NO_TEXEL;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const float r = rgb[3 * (size_t)t], g = rgb[3 * (size_t)t + 1], b = rgb[3 * (size_t)t + 2];
        if (env_texel_bad(r, g, b)) {
            bad = bad < t ? bad : t;
        } else {
            m = gmax(m, env_importance(r, g, b, env_row_sin(t / W, dth)));
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        m = gmax(m, __shfl_xor(m, off));
        const uint32_t ob = (uint32_t)__shfl_xor((int)bad, off);
        bad = bad < ob ? bad : ob;
    }
    if (bad != ENV_NO_TEXEL && (threadIdx.x & 63u) == 0u) atomicMin(&fl->bad_texel, bad);
    if ((threadIdx.x & 63u) == 0u) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < ENV_BLOCK / 64; ++w) m = gmax(m, wmax[w]);
        if (m > 0.0f) atomicMax(&fl->m_bits, bits_from_f(m));
    }
}

// One wave64 per row: 64 texels a step, an inclusive cross-lane scan of their weights and a
// carried sum.  Writes weight, the row's exclusive prefix (W + 1 words) and the row's sum.
__global__ __launch_bounds__(ENV_BLOCK) void k_env_rows(const float* __restrict__ rgb, uint32_t W, uint32_t H, float dth,
                                                        const EnvBuildFlags* fl, uint32_t* __restrict__ weight,
                                                        uint32_t* __restrict__ row_cdf, uint32_t* __restrict__ rowsum) {
    const uint32_t j = blockIdx.x * (ENV_BLOCK / 64) + (threadIdx.x >> 6);
    if (j >= H) return;   // whole waves leave: the exchanges below are among a row's own lanes
    const uint32_t lane = threadIdx.x & 63u;
    const float m = f_from_bits(fl->m_bits);
    const float sj = env_row_sin(j, dth);
    uint32_t* row = row_cdf + (size_t)j * (W + 1u);
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < W; base += 64u) {
        const uint32_t i = base + lane;
        uint32_t w = 0u;
        if (i < W) {
            const float* p = rgb + 3 * ((size_t)j * W + i);
            w = env_weight(env_importance(p[0], p[1], p[2], sj), m);
        }
        uint32_t incl = w;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
            if (lane >= (uint32_t)off) incl += up;
        }
        if (i < W) {
            weight[(size_t)j * W + i] = w;
            row[i] = carry + (incl - w);
        }
        carry += (uint32_t)__shfl((int)incl, 63);
    }
    if (lane == 0u) {
        row[W] = carry;
        rowsum[j] = carry;
    }
}

// One block over the H row sums: ENV_BLOCK at a step, a scan through LDS and a carried sum.
__global__ __launch_bounds__(ENV_BLOCK) void k_env_marginal(const uint32_t* __restrict__ rowsum, uint32_t H,
                                                            uint64_t* __restrict__ marginal) {
    __shared__ uint64_t sc[2][ENV_BLOCK];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < H; base += ENV_BLOCK) {
        const uint32_t j = base + threadIdx.x;
        const uint64_t v = j < H ? (uint64_t)rowsum[j] : 0ull;
        int cur = 0;
        sc[0][threadIdx.x] = v;
        __syncthreads();
        for (uint32_t off = 1; off < ENV_BLOCK; off <<= 1) {
            uint64_t x = sc[cur][threadIdx.x];
            if (threadIdx.x >= off) x += sc[cur][threadIdx.x - off];
            sc[cur ^ 1][threadIdx.x] = x;
            cur ^= 1;
            __syncthreads();
        }
        const uint64_t incl = sc[cur][threadIdx.x];
        if (j < H) marginal[j] = carry + (incl - v);
        carry += sc[cur][ENV_BLOCK - 1];
        __syncthreads();   // sc is reused by the next step
    }
    if (threadIdx.x == 0u) marginal[H] = carry;
}

// khp_debug_env_light: the sampler over draws and the evaluation over dir_in, one item per thread.
__global__ __launch_bounds__(ENV_BLOCK) void k_dbg_env_light(const EnvLight* Ep, uint32_t n, const float* draws,
                                                             const float* dir_in, float* s_dir, float* s_pdf,
                                                             float* s_rad, int32_t* s_valid, float* e_rad, float* e_pdf) {
    const EnvLight E = *Ep;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        v3 d, L;
        float p;
        uint32_t texel;
        bool ok;
        env_light_sample(E, draws[2 * (size_t)k], draws[2 * (size_t)k + 1], d, L, p, texel, ok);
        s_dir[3 * (size_t)k] = d.x; s_dir[3 * (size_t)k + 1] = d.y; s_dir[3 * (size_t)k + 2] = d.z;
        s_rad[3 * (size_t)k] = L.x; s_rad[3 * (size_t)k + 1] = L.y; s_rad[3 * (size_t)k + 2] = L.z;
        s_pdf[k] = p;
        s_valid[k] = ok ? 1 : 0;
        env_light_eval(E, ld3(dir_in + 3 * (size_t)k), L, p, texel);
        e_rad[3 * (size_t)k] = L.x; e_rad[3 * (size_t)k + 1] = L.y; e_rad[3 * (size_t)k + 2] = L.z;
        e_pdf[k] = p;
    }
}

static void swap_mem(DevMem& a, DevMem& b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
}

extern "C" khp_status khp_get_env_light(khp_ctx* c, khp_env_light* out) {
    if (!c || !out) return fail(KHP_EINVAL, "khp_get_env_light: null argument");
    *out = c->env_light;
    return KHP_OK;
}

// Copies the map into memory of the context's own, checks it and builds the table, all in
// allocations that replace the context's only once nothing can fail any more.  Nothing of the
// tree is rebuilt: the ENV kernel instances read the light through S.envl.
extern "C" khp_status khp_set_env_light(khp_ctx* c, const khp_env_light* p) {
    if (!p) return fail(KHP_EINVAL, "khp_set_env_light: null argument");
    const bool off = p->width == 0u && p->height == 0u;
    if (!off) {
        if (const char* why = env_light_param_error(p)) return fail(KHP_EINVAL, std::string("khp_set_env_light: ") + why);
    } else if (p->reserved != 0u) {
        return fail(KHP_EINVAL, "khp_set_env_light: reserved must be 0");
    }
    if (!c) return fail(KHP_EINVAL, "khp_set_env_light: ctx is null");
    const bool device_map = (p->flags & KHP_ENV_LIGHT_DEVICE) != 0u;
    if (!off && c->bd.enabled)
        return fail(KHP_EUNSUPPORTED, "khp_set_env_light: the light-path variant knows KIRK's lights only: disable khp_set_bdpt first");
    if (!off && c->S.hair_lobes != HAIR_LOBE_R)
        return fail(KHP_EUNSUPPORTED, "khp_set_env_light: TT / TRT lobes are not traced under the environment light: khp_set_hair_lobes(R) first");
    if (!off && !device_map) {
        const std::string bad = env_light_texel_error(p->rgb, p->width, p->height);
        if (!bad.empty()) return fail(KHP_EINVAL, "khp_set_env_light: " + bad);
    }
    HIPCHK(hipSetDevice(c->device));
    KHPCHK(drain(c));   // frames in flight finish with the light they started with
    if (off) {
        c->S.envl = nullptr;
        khp_env_light_defaults(&c->env_light);
        ++c->gen;
        return KHP_OK;
    }
    const uint32_t W = p->width, H = p->height;
    const size_t n = (size_t)W * H;
    DevMem rgb, weight, row_cdf, marginal, rowsum, flags, dev;
    HIPCHK(rgb.ensure(12 * n));
    HIPCHK(weight.ensure(4 * n));
    HIPCHK(row_cdf.ensure(4 * (size_t)(W + 1u) * H));
    HIPCHK(marginal.ensure(8 * ((size_t)H + 1u)));
    HIPCHK(rowsum.ensure(4 * (size_t)H));
    HIPCHK(flags.ensure(sizeof(EnvBuildFlags)));
    HIPCHK(dev.ensure(sizeof(EnvLight)));
    HIPCHK(hipMemcpyAsync(rgb.p, p->rgb, 12 * n, device_map ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    const EnvBuildFlags f0{0u, ENV_NO_TEXEL};
    HIPCHK(hipMemcpyAsync(flags.p, &f0, sizeof f0, hipMemcpyHostToDevice, c->stream));
    const float dth = env_dth(H);
    const uint32_t grid_max = std::min((uint32_t)((n + ENV_BLOCK - 1) / ENV_BLOCK), 1024u);
    hipLaunchKernelGGL(k_env_max, dim3(grid_max), dim3(ENV_BLOCK), 0, c->stream, rgb.as<float>(), W, H, dth,
                       flags.as<EnvBuildFlags>());
    HIPCHK(hipGetLastError());
    EnvBuildFlags f1{};
    HIPCHK(hipMemcpyAsync(&f1, flags.p, sizeof f1, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the environment light's map check"));
    if (f1.bad_texel != ENV_NO_TEXEL)
        return fail(KHP_EINVAL, "khp_set_env_light: texel (" + std::to_string(f1.bad_texel % W) + ", " +
                                    std::to_string(f1.bad_texel / W) + ") is negative or not finite");
    if (f1.m_bits == 0u) return fail(KHP_EINVAL, "khp_set_env_light: the map is black");
    const uint32_t rows_per_block = ENV_BLOCK / 64;
    hipLaunchKernelGGL(k_env_rows, dim3((H + rows_per_block - 1) / rows_per_block), dim3(ENV_BLOCK), 0, c->stream,
                       rgb.as<float>(), W, H, dth, flags.as<EnvBuildFlags>(), weight.as<uint32_t>(),
                       row_cdf.as<uint32_t>(), rowsum.as<uint32_t>());
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_env_marginal, dim3(1), dim3(ENV_BLOCK), 0, c->stream, rowsum.as<uint32_t>(), H,
                       marginal.as<uint64_t>());
    HIPCHK(hipGetLastError());
    EnvLight E{};
    E.W = W;
    E.H = H;
    E.nee = p->nee;
    E.scale = p->scale;
    E.rotation = p->rotation;
    E.select = p->select;
    E.dth = dth;
    E.dph = env_dph(W);
    E.rgb = rgb.as<float>();
    E.weight = weight.as<uint32_t>();
    E.row_cdf = row_cdf.as<uint32_t>();
    E.marginal = marginal.as<uint64_t>();
    HIPCHK(hipMemcpyAsync(dev.p, &E, sizeof E, hipMemcpyHostToDevice, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the environment light's table build"));
    swap_mem(c->envl_rgb, rgb);
    swap_mem(c->envl_weight, weight);
    swap_mem(c->envl_row_cdf, row_cdf);
    swap_mem(c->envl_marginal, marginal);
    swap_mem(c->envl_dev, dev);
    c->S.envl = c->envl_dev.as<EnvLight>();
    c->env_light = *p;
    c->env_light.flags = 0u;
    c->env_light.rgb = nullptr;
    ++c->gen;
    return KHP_OK;
}

extern "C" khp_status khp_debug_env_light_tables(khp_ctx* c, uint32_t* weight, uint32_t* row_cdf, uint64_t* marginal) {
    if (!c || !weight || !row_cdf || !marginal) return fail(KHP_EINVAL, "khp_debug_env_light_tables: null argument");
    if (!c->S.envl) return fail(KHP_ENOTREADY, "khp_debug_env_light_tables: khp_set_env_light first");
    KHPCHK(drain(c));
    HIPCHK(hipSetDevice(c->device));
    const size_t W = c->env_light.width, H = c->env_light.height;
    HIPCHK(hipMemcpyAsync(weight, c->envl_weight.p, 4 * W * H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(row_cdf, c->envl_row_cdf.p, 4 * (W + 1) * H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(marginal, c->envl_marginal.p, 8 * (H + 1), hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the environment light's table query"));
    return KHP_OK;
}

extern "C" khp_status khp_debug_env_light(khp_ctx* c, uint32_t n, const float* draws, const float* dir_in, float* s_dir,
                                          float* s_pdf, float* s_radiance, int32_t* s_valid, float* e_radiance,
                                          float* e_pdf) {
    if (!c || !draws || !dir_in || !s_dir || !s_pdf || !s_radiance || !s_valid || !e_radiance || !e_pdf)
        return fail(KHP_EINVAL, "khp_debug_env_light: null argument");
    if (n == 0u || n > DBG_MAX_ITEMS) return fail(KHP_EINVAL, "khp_debug_env_light: n must be in [1, 2^20]");
    if (!c->S.envl) return fail(KHP_ENOTREADY, "khp_debug_env_light: khp_set_env_light first");
    KHPCHK(drain(c));
    HIPCHK(hipSetDevice(c->device));
    DevMem dd, di, od, op, orad, ov, er, ep;
    HIPCHK(upload(dd, draws, 2 * (size_t)n, c->stream));
    HIPCHK(upload(di, dir_in, 3 * (size_t)n, c->stream));
    HIPCHK(od.ensure(12 * (size_t)n));
    HIPCHK(op.ensure(4 * (size_t)n));
    HIPCHK(orad.ensure(12 * (size_t)n));
    HIPCHK(ov.ensure(4 * (size_t)n));
    HIPCHK(er.ensure(12 * (size_t)n));
    HIPCHK(ep.ensure(4 * (size_t)n));
    hipLaunchKernelGGL(k_dbg_env_light, dim3(dbg_grid(n)), dim3(ENV_BLOCK), 0, c->stream, c->S.envl, n, dd.as<float>(),
                       di.as<float>(), od.as<float>(), op.as<float>(), orad.as<float>(), ov.as<int32_t>(), er.as<float>(),
                       ep.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s_dir, od.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(s_pdf, op.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(s_radiance, orad.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(s_valid, ov.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(e_radiance, er.p, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(e_pdf, ep.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    KHPCHK(wait_stream(c, c->stream, "the environment light queries"));
    return KHP_OK;
}
