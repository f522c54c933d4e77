/*
 * kirk_hip.h -- C-ABI of the MI355X-native fur path-tracing core.
 *
 * This is the drop-in boundary for the hot path of lucashilbig/BA_Pathtracing_Fur
 * ("KIRK"): camera ray -> BVH closest hit over hair cone frusta and triangles ->
 * shader/BSDF -> next-event shadow ray -> accumulate.  Every entry point below
 * replaces one KIRK C++ interface; the replaced interface is cited (file:line,
 * relative to the KIRK source tree src/libraries/KIRK/).
 *
 * Conventions
 *  - plain C: no exceptions cross the ABI, no C++ or torch types in signatures;
 *  - every call returns a khp_status; khp_last_error() returns a thread-local
 *    message for the last failing call of this thread;
 *  - all inputs are host pointers and are copied; outputs are caller-owned;
 *  - one khp_ctx is single-threaded, like KIRK's non-re-entrant
 *    CPU_Raytracer::render (KIRK/Utils/Threading.h:117);
 *  - internally: one HIP device + one stream per context, optional RCCL comm.
 *
 * Coordinates/units are KIRK's: world space, right-handed, y up; images are
 * stored row-major with row 0 at the BOTTOM of the frame (Camera::getRayFromPixel
 * starts at m_bottom_left, KIRK/Common/Camera.cpp:59-66).
 */
#ifndef KIRK_HIP_H
#define KIRK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KHP_ABI_VERSION 17

typedef struct khp_ctx khp_ctx;

typedef enum {
    KHP_OK = 0,
    KHP_EINVAL = 1,       /* bad argument (KIRK: std::invalid_argument)          */
    KHP_ENOMEM = 2,       /* host or device allocation failed                   */
    KHP_EDEVICE = 3,      /* HIP / RCCL error, or no device                     */
    KHP_ENOTREADY = 4,    /* call order violated (e.g. render before build)     */
    KHP_EUNSUPPORTED = 5  /* feature outside the hot path (textures, env maps)  */
} khp_status;

/* ---------------------------------------------------------------------------
 * BSDF and shader kinds.  KIRK registers BSDFs by name in a singleton factory
 * (Bsdf.h:133-241, BsdfFactory.cpp:28-55) and binds std::function callbacks;
 * callbacks cannot run on a GPU, so the GPU side is a closed enum keyed by the
 * same names (khp_bsdf_kind_from_name).
 * ------------------------------------------------------------------------- */
typedef enum {
    KHP_BSDF_LAMBERTIAN_REFLECTION = 0,   /* "LambertianReflectionBSDF"   Bsdf.cpp:186-202 */
    KHP_BSDF_SPECULAR_REFLECTION = 1,     /* "SpecularReflectionBSDF"     Bsdf.cpp:210-219 */
    KHP_BSDF_SPECULAR_TRANSMISSION = 2,   /* "SpecularTransmissionBSDF"   Bsdf.cpp:258-290 */
    KHP_BSDF_GLOSSY = 3,                  /* "GlossyBSDF"                 Bsdf.cpp:227-250 */
    KHP_BSDF_GLASS = 4,                   /* "GlassBSDF"                  Bsdf.cpp:326-359 */
    KHP_BSDF_MILK_GLASS = 5,              /* "MilkGlassBSDF"              Bsdf.cpp:367-418 */
    KHP_BSDF_LAMBERTIAN_TRANSMISSION = 6, /* "LambertianTransmissionBSDF" Bsdf.cpp:298-318 */
    KHP_BSDF_EMISSION = 7,                /* "EmissionBSDF"               Bsdf.cpp:427-437 */
    KHP_BSDF_TRANSPARENT = 8,             /* "TransparentBSDF"            Bsdf.cpp:445-456 */
    KHP_BSDF_MARSCHNER_HAIR = 9,          /* "MarschnerHairBSDF"          Bsdf.cpp:465-776 */
    KHP_BSDF_DEON_HAIR = 10,              /* "DEonHairBSDF"               Bsdf.cpp:784-1056 */
    KHP_BSDF_CHIANG_HAIR = 11,            /* "ChiangHairBSDF": not KIRK's; khp_hair_material below */
    KHP_BSDF_COUNT = 12
} khp_bsdf_kind;

typedef enum {
    KHP_SHADER_SIMPLE = 0,          /* "SimpleShader"        SimpleShader.h:31-152        */
    KHP_SHADER_MARSCHNER_HAIR = 1,  /* "MarschnerHairShader" MarschnerHairShader.h:31-138 */
    KHP_SHADER_COUNT = 2
} khp_shader_kind;

/* KIRK::Material (Material.h:53-152): the parameter values.  Textured
 * parameters (MatParamColor/MatParamFloat with a texture) are given by
 * khp_scene.material_textures below (ABI 6). */
typedef struct {
    int32_t bsdf;          /* khp_bsdf_kind   */
    int32_t shader;        /* khp_shader_kind */
    float diffuse[3];      /* m_diffuse   */
    float specular[3];     /* m_specular  */
    float volume[3];       /* m_volume    */
    float emission[3];     /* m_emission  */
    float ior;             /* m_ior (KIRK default 1.52, Material.h:83)    */
    float roughness;       /* m_roughness (KIRK default 1.0)             */
} khp_material;

typedef enum {
    KHP_LIGHT_POINT = 0,   /* PointLight Light.cpp:127-199 */
    KHP_LIGHT_QUAD = 1,    /* QuadLight  Light.cpp:216-296 */
    KHP_LIGHT_SPOT = 2,    /* SpotLight  Light.cpp:327-440 */
    KHP_LIGHT_SUN = 3      /* SunLight   Light.cpp:463-511 */
} khp_light_kind;

/* Constructor arguments of the KIRK light classes (Light.h), identity node
 * transform.  The library derives the same state KIRK derives in the ctor
 * and in Light::transform (normalised direction, quad vertices). */
typedef struct {
    int32_t kind;          /* khp_light_kind */
    float color[3];
    float position[3];
    float direction[3];    /* ctor argument; normalised by the library      */
    float size[2];         /* QuadLight m_size                               */
    float radius;          /* point/spot/sun m_radius                        */
    float att_const, att_lin, att_quad;
    float inner_angle, outer_angle;   /* SpotLight, degrees                  */
} khp_light;

/* KIRK::Environment (Environment.h): background colour + ambient.  The
 * CUBE_MAP / SPHERE_MAP types are khp_scene.env_map (ABI 6). */
typedef struct {
    float color[3];
    float ambient[3];
} khp_environment;

/* ABI 6: KIRK::Texture as the CPU path tracer reads it (Texture.cpp:243-287):
 * 8-bit texels, 1..4 channels, row y at data + y * width * channels (KIRK's
 * m_texture_data), looked up nearest-texel with KIRK's wrap rule. */
#define KHP_TEX_WRAP_CLAMP 0   /* TEXTURE_WRAP_MODE_CLAMP (Texture.h:34) */
#define KHP_TEX_WRAP_TILE 1    /* TEXTURE_WRAP_MODE_TILE  (Texture.h:35), KIRK's default */
typedef struct {
    uint32_t width, height;
    uint32_t channels;         /* 1 (rrrr), 2 (rrrg), 3 (rgb1) or 4 (rgba)         */
    uint32_t wrap_mode;        /* m_texture_wrap_mode                              */
    const uint8_t* data;       /* width * height * channels bytes, copied          */
} khp_texture;

/* ABI 6: which material parameters are textured (index into khp_scene.textures,
 * -1: the khp_material value).  Material::getFromParam (Material.cpp:15-23):
 * colours take the texel's rgb, roughness takes the length of its rgba. */
typedef struct {
    int32_t diffuse, specular, volume, emission, roughness;
} khp_material_textures;

/* ABI 6: Environment::m_type (Environment.h:25-30, getColor Environment.cpp:91-133). */
#define KHP_ENV_COLOR 0
#define KHP_ENV_CUBE_MAP 1     /* tex: posx, posy, posz, negx, negy, negz (loadCubeMap order) */
#define KHP_ENV_SPHERE_MAP 2   /* tex[0] */
typedef struct {
    int32_t type;
    int32_t tex[6];            /* indices into khp_scene.textures                  */
} khp_env_map;

/* The state KIRK::Camera::applyParameters derives (Camera.cpp:6-37). */
typedef struct {
    float position[3];
    float bottom_left[3];
    float axis_x[3];
    float axis_y[3];
    float pixel_size;
} khp_camera;

/* Flattened scene = what KIRK::CPU::Scene::flattenNode produces
 * (CPU_Scene.cpp:73-197), before the Triangle/Cylinder constructors run.
 * Object order (it shapes the BVH): triangles [0,n_tris) then cones. */
typedef struct {
    uint32_t n_tris;
    const float* tri_v;           /* [n_tris][3][3] vertices a,b,c (Triangle ctor args) */
    const float* tri_n;           /* [n_tris][3][3] vertex normals na,nb,nc             */
    const uint32_t* tri_mat;      /* [n_tris] material index                            */
    uint32_t n_cones;
    const float* cone_base_r0;    /* [n_cones][4] basePoint.xyz, baseRadius  (Cylinder ctor) */
    const float* cone_apex_r1;    /* [n_cones][4] apexPoint.xyz, apexRadius                  */
    const uint32_t* cone_mat;     /* [n_cones] material index                                */
    uint32_t n_materials;
    const khp_material* materials;
    uint32_t n_lights;
    const khp_light* lights;
    khp_environment env;
    khp_camera camera;
    /* ABI 4: optional [n_tris][3][3] hair frame u, v, w per triangle
     * (Object::setU/V/W, set by CPU_Scene::fiberToTriangles, CPU_Scene.cpp:
     * 232-345, for fur drawn as triangle tubes; read by the hair BSDFs).
     * NULL: zero frames (KIRK leaves them uninitialised on plain triangles). */
    const float* tri_frame;
    /* ABI 6: node transforms of the cones.  flattenNode hands each fiber's
     * Cylinder the transform base_transform * child->m_transform
     * (CPU_Scene.cpp:119, 136-137); the ctor maps base/apex by it and the frame
     * by its inverse transpose (Cylinder.cpp:5-29).  cone_base_r0/apex_r1 are
     * then the PRE-transform points.  n_cone_models = 0: world-space cones
     * (identity, the ctor's arithmetic without the matrix products). */
    uint32_t n_cone_models;
    const float* cone_models;     /* [n_cone_models][16] glm::mat4, column-major             */
    const uint32_t* cone_model;   /* [n_cones] index into cone_models; NULL: model 0 for all */
    /* ABI 6: textures (a17 / a16 / a9 in SURVEY §8) */
    uint32_t n_textures;
    const khp_texture* textures;
    const khp_material_textures* material_textures;  /* [n_materials], or NULL: untextured */
    const float* tri_uv;          /* [n_tris][3][2] texcoords tca, tcb, tcc, or NULL: zeros   */
    khp_env_map env_map;          /* type KHP_ENV_COLOR: env.color (zero-initialised = COLOR) */
} khp_scene;

#define KHP_RENDER_OUT_DEVICE   (1u << 0)  /* out_rgb is a device pointer        */
#define KHP_RENDER_NO_READBACK  (1u << 1)  /* keep framebuffer in HBM only       */
#define KHP_RENDER_STATS        (1u << 2)  /* instrumented kernels for this call  */
#define KHP_RENDER_ASYNC        (1u << 3)  /* enqueue and return (ABI 5): frames in flight overlap;
                                              no readback, no STATS; khp_sync completes them */

/* One khp_render call = samples [first_sample, first_sample+spp) of
 * PathTracer::render (CPU_PathTracer.cpp:17-52) for every pixel this rank
 * owns; the framebuffer holds KIRK's running mean (drawTexture, :61-90). */
typedef struct {
    uint32_t width, height;
    uint32_t spp;            /* samples in this call                               */
    uint32_t depth;          /* max bounces, PathTracer m_depth (Demo uses 5)      */
    uint32_t seed;           /* frame seed of the counter RNG                      */
    uint32_t first_sample;   /* progressive resume: 0 starts a new frame           */
    uint32_t tile_size;      /* square tiles; 0 -> 64                              */
    uint32_t tile_rank;      /* this rank renders tiles with id % tile_nranks == tile_rank */
    uint32_t tile_nranks;    /* 0 or 1 -> all tiles                                */
    uint32_t flags;          /* KHP_RENDER_*                                       */
} khp_render_params;

typedef struct {
    uint64_t n_objects, n_nodes, n_leaves;
    uint32_t bvh_depth, max_leaf_size;
    uint64_t device_bytes;           /* scene + BVH + queues resident in HBM  */
    double build_ms;                 /* flatten + BVH build (host)            */
    double upload_ms;
    double render_ms;                /* last khp_render, device time          */
    double extend_ms, shade_ms, shadow_ms, other_ms;  /* per-kernel device time, last render */
    uint64_t extend_rays, shadow_rays, extend_launches;
    uint64_t node_visits, prim_tests, shadow_node_visits, shadow_prim_tests; /* KHP_CTX_STATS only */
    uint64_t stack_spills;           /* traversal-stack entries spilled from LDS (stats only) */
    /* per bounce (index = bounce, up to KHP_MAX_BOUNCE_STATS), instrumented renders only */
    uint64_t bounce_rays[16], bounce_nodes[16], bounce_prims[16];
    uint64_t bounce_shadow_rays[16], bounce_shadow_nodes[16], bounce_shadow_prims[16];
    double bounce_extend_ms[16], bounce_shadow_ms[16];
    /* traversal-loop efficiency (instrumented renders): wave iterations and the
     * lanes that had a record to fetch in them (busy / (64 * iters) = lane use) */
    uint64_t bounce_wave_iters[16], bounce_lanes_busy[16];
    uint64_t bounce_shadow_wave_iters[16], bounce_shadow_lanes_busy[16];
    /* diagnostic builds (KHP_PROFILE_STEPS=1) only: k_extend wave cycles spent in
     * resolve / record fetch / compute / loop+refill, summed over waves */
    uint64_t step_cycles[4];
    /* ABI 3: where khp_build_accel built the BVH and how long it took */
    uint32_t bvh_on_device;          /* 1: device build (default), 0: host   */
    uint32_t subframes;              /* always 1 (ABI 6: one path set per frame slot) */
    double flatten_ms;               /* khp_set_scene (flatten, incl. copies) */
    double bvh_ms;                   /* BVH build wall time incl. transfers   */
    double bvh_kernel_ms;            /* device build: GPU time of its kernels  */
    double layout_ms;                /* node pairing + leaf slots + slot records */
    double flatten_kernel_ms;        /* device flatten: GPU time of its kernels */
    double layout_kernel_ms;         /* device layout: GPU time of its kernels  */
    /* stack entries popped only to fail the prune test (instrumented renders) */
    uint64_t extend_pruned_pops, shadow_pruned_pops;
    /* ABI 5: frames this report covers -- 1 after a synchronous khp_render (1 +
     * render_ahead when the call rendered the next calls' passes in its fused
     * batch, whose timings and counters it then reports); after khp_sync, every
     * asynchronous frame completed since the previous report, with timings
     * (extend_ms, extend_launches, ...) and counters summed over them */
    uint64_t frames;
    /* ABI 5: wall time during which at least one k_extend launch of the report
     * was running (union of the launches' HIP-event intervals); equals extend_ms
     * when launches do not overlap (synchronous renders) */
    double extend_busy_ms;
    /* ABI 6: the shadow stage split -- shadow_ms above is k_shadow + the shadow
     * finish; shadow_finish_ms is the finish alone, shadow_launches counts the
     * any-hit (k_shadow) launches */
    double shadow_finish_ms;
    uint64_t shadow_launches;
    /* ABI 13: render-ahead (khp_ctx_params.render_ahead), last synchronous render:
     * its paths earlier calls had already finished (all of them when an earlier
     * wavefront call's fused batch held its pass), and those it resumed from park
     * records (0 when the call had nothing rendered ahead) */
    uint64_t ahead_finished, ahead_resumed;
} khp_stats;
#define KHP_MAX_BOUNCE_STATS 16

#define KHP_CTX_STATS  (1u << 0)   /* instrumented kernels: count node/prim visits */
#define KHP_CTX_HOST_BUILD (1u << 1) /* khp_build_accel builds the BVH on the host
                                       (default: on the device, the same tree)   */

/* ABI 6: scheduling parameters of a context.  They decide how the wavefront
 * is cut and overlapped on the device, never what it computes: every value
 * gives the same frames bit for bit.  khp_ctx_params_defaults() fills the
 * measured defaults; khp_set_params completes in-flight frames
 * first.  (KIRK has no counterpart: its PathTracer segments by the GUI's
 * maxBufferSize, CPU_PathTracer.cpp:211-241, which chunk_paths mirrors.) */
typedef struct {
    uint32_t fuse_frames;        /* asynchronous frames with equal parameters fused into one batch,
                                    1..32 (default 32)                                               */
    uint32_t frames_in_flight;   /* batches in flight at once, 1..3 (default 1)                     */
    uint64_t chunk_paths;        /* paths per wavefront chunk, >= 4096; 0 (default): the smaller of
                                    2^28 (2^27 before round 6) and what fits in half the free HBM    */
    uint32_t heavy_iters;        /* longest-first queues: a path whose last traversal took more
                                    iterations has its next rays claimed first (default 0xFFFFFFFF =
                                    off since round 6; 160 before).  No effect on the extension rays
                                    of bounces regrouped by ray_sort_from (their claim order is the
                                    cell order; shadow rays keep it); path_order 2 marks its heavy
                                    pixels with it                                                  */
    int32_t dump_bounce;         /* debug: keep the extension rays of this bounce of the next
                                    synchronous render for khp_debug_queue (-1: off, default)       */
    uint32_t trace_kernels;      /* khp_trace_closest / khp_trace_any run on 0: one-ray-per-thread
                                    kernels (default), 1: the instrumented persistent kernels (KIRK's
                                    visit counts), 2: the production persistent kernels.  With 1 or
                                    2 a query fails with KHP_EDEVICE if a result of the batch was
                                    never written or a slot past the batch was (test hook)          */
    uint32_t shade_order;        /* ABI 7: 0 (default): k_shade takes the hits in queue order; 1: hits are
                                    first grouped by shading class (no hit / BSDF kind), a counting
                                    sort per bounce -- KIRK's GLSL template only compacts its hits
                                    (pt_sortHits.compute:17-38); measured in DESIGN.md §4            */
    uint32_t serial_stages;      /* ABI 7: 1 = the shadow stage runs on the extend stream, so no two
                                    kernels of a frame overlap and each kernel's timing is its own
                                    (bench.py's isolated per-kernel rooflines); 0 (default) = two
                                    streams, shadow stage b beside extend b+1                         */
    uint32_t path_order;         /* ABI 9: how a fused chunk numbers its paths.  0: frame-major (frame f's
                                    pixels x samples form one block); 1 (default): pixel-major (all fused
                                    frames' samples of one pixel are adjacent paths, so a wave traces one
                                    pixel of 8 frames at 8 spp); 2: pixel-major, and the wavefront takes the
                                    pixels whose previous camera ray was long first (a per-batch permutation
                                    of the pixel list; results unchanged).  Measured in DESIGN.md §5a   */
    uint32_t wide_from;          /* ABI 10: the first bounce whose closest-hit traversal runs on two-level
                                    node records (one 128-B record per step: a node's child boxes and the
                                    near child's own, KIRK's order and counts kept); earlier bounces use the
                                    64-B records.  Default 2 (measured); >= depth: never.
                                    The shadow stage (any hit) of bounce b uses them when b >= max(wide_from,
                                    2).  Batch queries with trace_kernels use them iff wide_from == 0   */
    uint32_t path_kernel;        /* ABI 11: 0 (default) automatic, 1 never, 2 whenever supported: run a chunk's
                                    paths through all their bounces in ONE persistent launch (k_path: a lane
                                    traces, shades, traces the shadow ray and continues with the next bounce)
                                    instead of the per-bounce wavefront, whose every launch ends with its
                                    slowest ray.  Automatic: synchronous renders (KIRK's own one-call-per-pass
                                    use) of at most 14 x 2^20 paths (1080p up to 7 spp; past that the
                                    wavefront's steady rate wins).  Not with the light-path variant, hit
                                    sorting, instrumented renders or queue dumps (those always run the
                                    wavefront).  Measured in DESIGN.md §5b                              */
    uint32_t ray_sort_from;      /* ABI 12: the first bounce whose extension rays are regrouped before
                                    k_extend by the Morton cell (32^3 over the scene box) of their origin, so
                                    that the rays of a claim block start close together and share cache
                                    lines; the path state stays in place.  Which lane traces which ray
                                    changes no result.  0 (default): automatic -- bounce 2 when the tree's
                                    node records exceed 64 MB, else never (a cache-resident tree has no
                                    misses to save; measured); 1..: that bounce; >= depth:
                                    never.  Not with hit sorting (shade_order 1), the light-path variant or
                                    queue dumps; the path kernel never sorts                              */
    uint32_t lds_nodes;          /* ABI 12: 0 (default) or 7: the tree's top three levels of node records
                                    staged in each traversal wave's LDS beside its stack rings (the 64-B
                                    loops of k_extend and k_shadow), the rest fetched from HBM as before.
                                    Same walk, same counts, same frames.  Measured in DESIGN.md §4    */
    uint32_t render_ahead;       /* ABI 13: 0..3 (default 3).  A synchronous render that runs the path kernel
                                    in one chunk lets the lanes that would idle in its launch's drain (its
                                    longest paths finishing alone) start the paths of the next render_ahead
                                    calls of a progressive series -- the same pixels, spp, depth and seed,
                                    first_sample + spp, + 2 spp, ...: KIRK's PathTracer::render loop,
                                    CPU_PathTracer.cpp:17-52.  A call still returns as soon as its own
                                    paths end (at once when earlier calls finished them all); the paths of
                                    later calls in flight then are parked and resumed by later calls, which
                                    accumulate the colours already finished.  Any other call, and any change
                                    of scene, camera or parameters, drops that work.  A synchronous render
                                    that runs the wavefront (one chunk) and continues the series of the
                                    previous synchronous call renders its own pass and the next render_ahead
                                    calls' passes as one fused batch; those calls then only accumulate.
                                    Frames, textures and framebuffers are those of each call alone, bit for
                                    bit.  Measured in DESIGN.md §5c                                        */
    uint32_t path_from;          /* ABI 13: 0 (default) or b >= 1: a wavefront render hands the paths still
                                    alive at bounce b to ONE path-kernel launch (k_path), which carries them
                                    through the remaining bounces without a barrier per bounce -- the last
                                    bounces' launches are short and end with their slowest ray.  Not with the
                                    light-path variant, hit sorting, instrumented renders or queue dumps;
                                    >= depth: off.  No value changes a pixel.  Measured in DESIGN.md §5d   */
} khp_ctx_params;   /* 64 bytes */

/* ---- context --------------------------------------------------------------- */
/* device: HIP device ordinal (one process per GPU). */
khp_status khp_create(khp_ctx** out, int device, uint32_t flags);
void khp_destroy(khp_ctx* ctx);
const char* khp_last_error(void);
int khp_abi_version(void);
void khp_ctx_params_defaults(khp_ctx_params* out);
khp_status khp_set_params(khp_ctx* ctx, const khp_ctx_params* params);
khp_status khp_get_params(khp_ctx* ctx, khp_ctx_params* out);

/* Replaces CPU::Scene::setSceneGraph (CPU_Scene.cpp:25-43) + the Triangle and
 * Cylinder constructors (Triangle.cpp:3-129, Cylinder.cpp:5-67). Copies. */
khp_status khp_set_scene(khp_ctx* ctx, const khp_scene* scene);

/* Replaces BVH::addBaseDataStructure (CPU_BVH.cpp:16-44): binned SAH, 16 bins,
 * leaf threshold 1 (CPU_BVH.h:64); uploads scene + BVH to HBM. */
khp_status khp_build_accel(khp_ctx* ctx);

/* Replaces PathTracer::render (CPU_PathTracer.cpp:17-52).  out_rgb: W*H*3
 * floats (host unless KHP_RENDER_OUT_DEVICE, ignored with NO_READBACK).
 * Pixels of tiles not owned by this rank are left untouched. */
khp_status khp_render(khp_ctx* ctx, const khp_render_params* p, float* out_rgb);

/* ---- per-pixel first-hit feature buffers (AOVs) ------------------------------
 * What a denoiser or compositor wants beside the colour: for every pixel this
 * rank owns and the samples k = first_sample .. first_sample + spp - 1, the
 * camera rays khp_render traces for those samples (the context's current camera)
 * and the surface at their first hit.  A sample is a surface sample when its
 * closest object hit exists (the hit khp_trace_closest reports) and no light's
 * own intersection is nearer (t_light < t_hit ends the path on the light, as in
 * traceRay).  A surface sample contributes
 *   normal   the shading normal (khp_debug_surface's; not face-forwarded),
 *   tangent  the hit object's hair frame V (KHP_AOV_TANGENT_IS_FRAME_V),
 *   albedo   the resolved material's diffuse (textured scenes: the texel's),
 *   depth    the hit's t along the normalised ray,
 *   coverage 1;
 * any other sample contributes +0 to every channel.  Each float channel is
 * s / (float)spp, where s starts at +0 and takes the samples' values in
 * increasing k with float32 adds: normal, tangent, albedo and depth are
 * premultiplied by coverage, a host divides.  object is the object id of sample
 * first_sample (-1 when that is not a surface sample).  The result is a function
 * of the arguments alone (no atomics, no scheduling-dependent order).
 *
 * p as for khp_render: width, height, spp, seed, first_sample and tile_* are
 * used, depth is ignored, flags is 0 or KHP_RENDER_OUT_DEVICE (then every
 * pointer is device memory of ctx's GPU).  A NULL buffer is not computed; pixels
 * of tiles this rank does not own are left untouched (hosts assemble tiles by
 * khp_gather_plan).  KHP_EINVAL: another flag, every buffer NULL, spp == 0 or
 * above 2^24, width * height == 0, a null argument; KHP_ENOTREADY without a
 * scene or a tree.  The arguments are checked before the context is touched.
 *
 * The call renders nothing: framebuffer, sample counters, khp_stats, render-ahead
 * work and asynchronous frames (pending or in flight) are left as they are; it is
 * only queued behind what the context's stream holds, and returns when its
 * buffers are written.  KIRK has no counterpart. */
#define KHP_AOV_TANGENT_IS_FRAME_V 1   /* documentation only: tangent = the hit object's V axis */
typedef struct {
    float*   normal;    /* [H][W][3] or NULL */
    float*   albedo;    /* [H][W][3] or NULL */
    float*   tangent;   /* [H][W][3] or NULL */
    float*   depth;     /* [H][W]    or NULL */
    float*   coverage;  /* [H][W]    or NULL */
    int32_t* object;    /* [H][W]    or NULL */
} khp_aov_buffers;
khp_status khp_render_aov(khp_ctx* ctx, const khp_render_params* p, const khp_aov_buffers* out);

/* ---- guided a-trous denoiser over the feature buffers -------------------------
 * An edge-stopping a-trous wavelet filter (B3 spline taps h = {1/16, 1/4, 3/8,
 * 1/4, 1/16}, 5 x 5 per iteration, iteration i at step 1 << i) of an [H][W][3]
 * colour frame, guided by the planes khp_render_aov writes (full frames,
 * premultiplied by coverage; only read; object is ignored).  The result is one
 * float32 function of the arguments in a fixed order of operations, the same
 * bits from khp_denoise (gfx950 kernels) and khp_denoise_host (a plain host
 * loop): no atomics, nothing contracted.  The definition, operation by
 * operation, is DESIGN.md §13; in short
 *   prepare  per pixel: cv = coverage, n / t = normal / tangent divided by cv and
 *            normalised (0 where that has no length), d = depth / cv, c = colour,
 *            channels above `clamp` set to it, and with DEMODULATE c / m where
 *            m = max(albedo + (1 - cv), 1e-3) per channel;
 *   iterate  w = h[dy] h[dx] k_expf(-X) over the taps inside the image whose colour
 *            is finite, X the sum of the enabled squared distances (colour, normal,
 *            tangent, depth, coverage) each times 1 / sigma^2; the new colour is
 *            sum(w c_q) / sum(w) over the taps with w > 0, or the old one if none;
 *   finish   with DEMODULATE c * m.
 * A pixel that is not finite takes no part as a tap, has its colour term off and
 * is replaced by its neighbours' guided mean: it never spreads, and survives only
 * where no tap counts.  A sigma of 0 turns its term off; a plane whose term is
 * off is not read and may be NULL (coverage is also read whenever normal,
 * tangent, depth or albedo is).
 *
 * colour and out are [H][W][3] floats, out == colour is allowed.  khp_denoise
 * with colour == NULL filters the context's framebuffer (the running mean
 * khp_read_framebuffer returns; width and height must be its size): it completes
 * asynchronous frames as that call does, reads the framebuffer and writes
 * nothing of the context.  With a caller's colour the call touches no context
 * state (own scratch, queued on the context's stream, returns when out is
 * written), like khp_render_aov.  Whole frames only: a tile rank filters after
 * khp_gather_framebuffer.
 *
 * KHP_EINVAL (checked before the context is touched, khp_last_error names the
 * cause): a null p, guides, out or ctx; colour == NULL or KHP_DENOISE_DEVICE at
 * the host entry; width * height == 0 or above 2^31; iterations outside 1..8;
 * an unknown flag; reserved != 0; a sigma or clamp negative or not finite; a
 * term on whose plane is NULL; DEMODULATE without albedo; coverage NULL while
 * normal, tangent, depth or albedo is used.  KHP_ENOTREADY: colour == NULL
 * before any render.  KIRK has no counterpart. */
#define KHP_DENOISE_DEVICE     (1u << 0)  /* colour, the guide planes and out are device memory of ctx's GPU */
#define KHP_DENOISE_DEMODULATE (1u << 1)  /* filter colour / effective albedo, multiply back at the end     */
typedef struct {
    uint32_t width, height;
    uint32_t iterations;        /* 1..8; iteration i uses step 1 << i */
    uint32_t flags;             /* KHP_DENOISE_* */
    float sigma_color, sigma_normal, sigma_tangent, sigma_depth, sigma_coverage;  /* 0: the term is off */
    float clamp;                /* > 0: colour channels above it are set to it first; 0: off */
    uint32_t reserved[2];       /* 0 */
} khp_denoise_params;           /* 48 bytes */
void khp_denoise_params_defaults(khp_denoise_params* out);  /* 0 x 0, 5 iterations, flags 0, 4, 0.35, 0.35, 0.05, 0.25, clamp 0 */
khp_status khp_denoise(khp_ctx* ctx, const khp_denoise_params* p, const float* colour,
                       const khp_aov_buffers* guides, float* out);
khp_status khp_denoise_host(const khp_denoise_params* p, const float* colour,
                            const khp_aov_buffers* guides, float* out);   /* no device, no context */

/* ---- the same filter guided by measured variance --------------------------------
 * khp_denoise_var is khp_denoise's a-trous scheme with the colour distance divided,
 * per pixel, by the measured variance of that pixel's mean: sigma_color is then in
 * standard deviations of the pixel's own noise, not in radiance units, so the same
 * call is right at 4 samples per pixel and at 400.  The variance is filtered along
 * with the colour and can be returned.  p is khp_denoise's struct with the same
 * meanings but for sigma_color (0 still turns the term off); the same bits from
 * khp_denoise_var (gfx950 kernels) and khp_denoise_var_host.  The definition,
 * operation by operation, is DESIGN.md §17; what is not restated there is §13's.
 *   prepare  per pixel a variance v and a flag known.  PLANE: u = variance[p].
 *            MOMENTS and CONTEXT: n = count, nf = (float)n, s = (m2.r + m2.g) + m2.b,
 *            u = s / (nf * (nf - 1.0f)) when n >= 2 (rel_error's radicand).  known =
 *            (PLANE or n >= 2) and u finite and u >= 0; v = known ? u : +0.
 *   iterate  before the taps, per pixel: prefilter 0: kbar = known, vbar = v;
 *            prefilter 1: over the 3 x 3 taps at spacing 1 inside the image and known,
 *            weights g[dy] g[dx], g = {1/4, 1/2, 1/4}, dy outer and dx inner, vbar =
 *            sum(g v) / sum(g) WITHOUT the first tap holding the largest v (kept when
 *            it is the only known tap), kbar = sum(g) > 0.  The largest tap is left out,
 *            never subtracted.  The colour term is on iff sigma_color > 0, the pixel is
 *            finite and kbar; then a tap adds d2(c_p, c_q) * icv to X, icv = (1 /
 *            sigma_color^2) / (vbar + floor).  Along the taps that count and are known,
 *            va += (w * w) * v_q and wk += w; if any tap counted, known' = wk > 0 and
 *            v' = known' ? va / (wk * wk) : +0, else v and known stay.
 *   finish   out as khp_denoise without DEMODULATE; out_variance = known ? v : +inf.
 * With sigma_color == 0 out is khp_denoise's bit for bit.  A pixel whose variance is
 * unknown filters with its colour term off, like a pixel that is not finite.  One
 * firefly's huge variance does not loosen its neighbours' colour term (the trimmed
 * prefilter), so it does not spread; it is not repaired either: the clamp is khp_denoise's.
 *
 * KHP_DENOISE_DEVICE covers every pointer, variance, m2, count and out_variance
 * included.  KHP_DENOISE_DEMODULATE is KHP_EUNSUPPORTED here: a scalar variance has
 * no per-channel albedo division (and demodulation is off by default, Marschner's R
 * radiance not carrying the diffuse colour).  out == colour is allowed.
 *
 * KHP_NOISE_CONTEXT reads the context's moments state in place (khp_set_moments on,
 * width and height the framebuffer's); with it colour == NULL is the moments' mean,
 * finite everywhere, read in place too; a caller's colour is allowed.  With the other
 * sources colour == NULL is the framebuffer as for khp_denoise.  Either way the call
 * completes asynchronous frames first and writes nothing of the context; with a
 * caller's colour and another source it touches no context state.
 *
 * KHP_EINVAL (checked before the context is touched, khp_last_error names the cause):
 * khp_denoise's cases; a null noise; an unknown source or prefilter; reserved != 0;
 * a floor negative or not finite; the source's plane(s) NULL (planes of the other
 * sources are ignored and never read); KHP_NOISE_CONTEXT at the host entry or with
 * another size than the framebuffer's.  KHP_ENOTREADY: KHP_NOISE_CONTEXT with moments
 * off or nothing rendered.  KIRK has no counterpart. */
#define KHP_NOISE_PLANE   0u  /* variance: [H][W], the variance of the pixel's MEAN, channels summed */
#define KHP_NOISE_MOMENTS 1u  /* m2 [H][W][3] and count [H][W], as khp_read_moments writes them */
#define KHP_NOISE_CONTEXT 2u  /* khp_denoise_var only: the context's moments state, read in place */
typedef struct {
    uint32_t source;          /* KHP_NOISE_* */
    uint32_t prefilter;       /* 0: the pixel's own variance; 1 (default): trimmed 3 x 3 (above) */
    float    floor;           /* finite, >= 0; added to the variance before the divide (default 1e-6f) */
    uint32_t reserved;        /* 0 */
    const float*    variance; /* PLANE */
    const float*    m2;       /* MOMENTS */
    const uint32_t* count;    /* MOMENTS */
    float*          out_variance;  /* [H][W] or NULL: the filtered variance, +inf where unknown */
} khp_denoise_noise;          /* 48 bytes */
void       khp_denoise_noise_defaults(khp_denoise_noise* out);   /* PLANE, 1, 1e-6f, 0, NULLs */
khp_status khp_denoise_var(khp_ctx* ctx, const khp_denoise_params* p, const float* colour,
                           const khp_aov_buffers* guides, const khp_denoise_noise* noise, float* out);
khp_status khp_denoise_var_host(const khp_denoise_params* p, const float* colour,
                                const khp_aov_buffers* guides, const khp_denoise_noise* noise, float* out);

/* ---- temporal reprojection: carry a frame's history across a camera move --------
 * khp_set_camera starts the running mean over.  khp_reproject instead takes the frame
 * of the previous camera (the history: colour, its effective sample count `length`, its
 * variance and its khp_render_aov planes) and the current camera's frame, finds for
 * every current pixel where its first-hit point was in the history, and blends the two.
 * The scene is static between the frames; only the camera moves.  A stateless call: the
 * caller keeps the outputs as the next history.  One float32 function of the arguments
 * in a fixed order of operations, the same bits from khp_reproject (a gfx950 kernel) and
 * khp_reproject_host (a plain host loop): no atomics, nothing contracted.  The
 * definition, operation by operation, is DESIGN.md §18; in short, per pixel (x, y)
 *   locate   the ray through the pixel centre (x + 0.5, y + 0.5) of cur.camera as
 *            khp_render makes it, normalised; cv = coverage; a surface pixel (cv > 0) is
 *            the point at d = depth / cv on it, a background pixel the ray's direction,
 *            a point at infinity (a rotation moves it, a translation does not);
 *   project  through hist.camera (axis_x and axis_y at right angles, as khp_camera_setup
 *            makes them) to a continuous pixel position (fx, fy); motion = (fx - (x +
 *            0.5), fy - (y + 0.5)), or NaN, NaN where the point is not in front of the
 *            history camera;
 *   taps     the four bilinear taps around (fx - 0.5, fy - 0.5), dy outer and dx inner.  A
 *            tap counts iff it is inside the image, its weight is > 0, its colour is finite,
 *            its length is finite and > 0 and every enabled test passes: depth (both
 *            surfaces with |d_q - dist| <= depth_tol * dist, dist the point's distance from
 *            the history camera, or both background), normal and tangent (1 - dot of the
 *            unit vectors <= tol; skipped when either has no length), coverage (|cv - cv_q|
 *            <= tol), object (equal ids).  h, N, vh = the counted taps' weighted colour,
 *            length and variance (squared weights, over the taps whose variance is known);
 *   blend    Nc = min(N, max_history) (max_history 0: N), s = samples, alpha = s / (Nc +
 *            s): colour h + alpha * (c - h), length Nc + s, variance (1 - alpha)^2 vh +
 *            alpha^2 v_c.  A current pixel that is not finite takes h, Nc, vh (the history
 *            repairs it); where no tap counted (a disocclusion, or no history) the result
 *            is c, s, v_c; where neither is usable c as it is, length 0.
 * A variance is the variance of the pixel's mean, channels summed, as for KHP_NOISE_PLANE;
 * negative or not finite means unknown, and out.variance holds +inf there, so the plane
 * feeds khp_denoise_var unchanged.  A tolerance of 0 turns its test off; a plane whose
 * test is off is not read and may be NULL, except the current frame's depth and coverage,
 * which locate the pixel and are always needed.  The history's coverage is read whenever
 * depth, normal, tangent or coverage is tested.  albedo is never read.  With hist == NULL
 * every pixel is "no tap counted", motion is NaN and no test plane is read.
 *
 * Each output may be NULL (not all).  out.colour == cur.colour (and out.variance ==
 * cur.variance) is allowed: the current frame is read per pixel.  An output equal to a
 * plane of the history is refused: the history is gathered.  khp_reproject touches no
 * context state (framebuffer, moments, frames in flight, render-ahead, stats): it has its
 * own staging area, is queued on the context's stream and returns when the outputs are
 * written, like khp_denoise with a caller's colour.  KHP_REPROJECT_DEVICE: every pointer
 * of cur, hist and out is device memory of ctx's GPU.
 *
 * KHP_EINVAL (checked before the context is touched, khp_last_error names the cause): a
 * null p, cur, out or ctx; width * height == 0 or above 2^31; an unknown flag; reserved
 * != 0; samples not finite or <= 0; max_history or a tolerance negative or NaN; every
 * output NULL; a NULL colour; cur's depth or coverage NULL; with a history: its length
 * NULL, an enabled test whose plane is NULL in either frame, an output that is one of
 * its planes; KHP_REPROJECT_DEVICE at the host entry, or with a pointer that is not
 * device memory.  KIRK has no counterpart. */
#define KHP_REPROJECT_DEVICE       (1u << 0)  /* every plane of cur, hist and out is device memory of ctx's GPU */
#define KHP_REPROJECT_MATCH_OBJECT (1u << 1)  /* a tap counts only if its object id is the pixel's           */
typedef struct {
    uint32_t width, height;   /* offset 0, 4 */
    uint32_t flags;           /* 8: KHP_REPROJECT_* */
    float samples;            /* 12: the current frame's weight, its samples per pixel; finite, > 0 */
    float max_history;        /* 16: > 0: the history's length is capped at it before the blend; 0: no cap */
    float depth_tol;          /* 20: relative; 0: the test is off */
    float normal_tol;         /* 24: 1 - cos; 0: off */
    float tangent_tol;        /* 28: 1 - cos; 0: off */
    float coverage_tol;       /* 32: absolute; 0: off */
    uint32_t reserved[3];     /* 36: 0 */
} khp_reproject_params;       /* 48 bytes */
typedef struct {
    khp_camera camera;        /* offset 0: the camera the frame was rendered with */
    uint32_t reserved;        /* 52: 0 */
    const float* colour;      /* 56: [H][W][3] */
    const float* variance;    /* 64: [H][W] or NULL (every variance unknown) */
    const float* length;      /* 72: [H][W], the history frame only: the effective samples behind each pixel */
    khp_aov_buffers aov;      /* 80: the planes khp_render_aov wrote with that camera (only read) */
} khp_reproject_frame;        /* 128 bytes */
typedef struct {
    float* colour;            /* offset 0: [H][W][3] or NULL */
    float* length;            /* 8: [H][W] or NULL */
    float* variance;          /* 16: [H][W] or NULL; +inf where unknown */
    float* motion;            /* 24: [H][W][2] or NULL; history position minus pixel centre, in pixels */
} khp_reproject_out;          /* 32 bytes */
/* 0 x 0, flags 0, samples 1, max_history 32, depth 0.05, normal 0 (off), tangent 0.25,
 * coverage 0.5: starting values, not a measured optimum */
void       khp_reproject_params_defaults(khp_reproject_params* out);
khp_status khp_reproject(khp_ctx* ctx, const khp_reproject_params* p, const khp_reproject_frame* cur,
                         const khp_reproject_frame* hist /* nullable */, const khp_reproject_out* out);
khp_status khp_reproject_host(const khp_reproject_params* p, const khp_reproject_frame* cur,
                              const khp_reproject_frame* hist /* nullable */, const khp_reproject_out* out);   /* no device, no context */

/* ---- per-pixel sample moments: robust mean, variance, error plane --------------
 * An opt-in second accumulator beside the framebuffer.  Per pixel it holds n, the
 * count of finite samples, their mean, M2, their sum of squared deviations
 * (Welford), and bad, the count of rejected samples; all zero when made.  It is
 * folded by the launches that fold the running mean, in the same sample order,
 * whatever the schedule (synchronous or asynchronous, fused, chunked, rendered
 * ahead, in flight): the state is a function of the samples alone (no atomics;
 * DESIGN.md §14).  The fold of a sample colour x with global index k, every step
 * one float32 operation in the order written, nothing contracted:
 *   k == 0                    the state is first set to zero (the framebuffer's
 *                             own restart rule);
 *   a channel of x not finite bad += 1, nothing else;
 *   otherwise                 n += 1, nf = (float)n;
 *     n == 1                  mean = x (an assignment: -0 survives), m2 = +0;
 *     n > 1, per channel      d = x - mean; mean = mean + d / nf; e = x - mean;
 *                             m2 = m2 + d * e.
 * For a series from sample 0 with no rejected sample, mean goes through the
 * running mean's own operations: it equals the framebuffer bit for bit on every
 * pixel with bad == 0; where bad > 0 the framebuffer is not finite and mean is.
 * Finite but huge samples can overflow m2 to +inf or NaN; nothing is clamped.
 * The error plane is computed on read: s = (m2.r + m2.g) + m2.b, mu = (mean.r +
 * mean.g) + mean.b, rel_error = +inf where n < 2, else
 * sqrtf(s / (nf * (nf - 1.0f))) / (fabsf(mu) + 1e-3f): the relative standard
 * error of the pixel's mean with the channels summed.
 *
 * Off by default, and with it off nothing changes.  khp_set_moments completes
 * frames in flight first.  Enabling makes a zeroed state, allocated with the
 * framebuffer (at once if there is one) and made anew, zeroed, whenever the
 * framebuffer is (a size change); enabled in mid-series it counts only the
 * samples folded since.  Disabling frees it; setting the value it has is a
 * no-op.  KHP_EINVAL: a null argument, enabled > 1, reserved != 0.
 *
 * khp_read_moments completes asynchronous frames as khp_read_framebuffer does,
 * writes the non-NULL planes and changes nothing of the context.  KHP_EINVAL
 * (checked before the context is touched): a null ctx or out, every plane NULL,
 * an unknown flag; with KHP_MOMENTS_DEVICE a plane that is not device memory.
 * KHP_ENOTREADY: moments off, or nothing rendered yet.  Pixels of tiles this rank
 * does not own are never folded and read as zeros (count 0, rel_error +inf); a
 * host assembles ranks by khp_gather_plan.
 *
 * khp_moments_fold_host is the definition as a plain host loop over the same
 * functions the kernels compile: samples is [n_samples][n_pixels][3], sample s
 * has global index first_sample + s, the state planes mean, m2, count and bad are
 * read and written, rel_error (or NULL) is written at the end.  KHP_EINVAL: a
 * null argument or state plane other than rel_error, n_pixels == 0, first_sample +
 * n_samples overflowing.  n_samples == 0 only writes rel_error.  KIRK has no
 * counterpart. */
typedef struct { uint32_t enabled; uint32_t reserved[3]; } khp_moments;      /* 16 bytes; reserved 0 */
void       khp_moments_defaults(khp_moments* out);                          /* off */
khp_status khp_set_moments(khp_ctx* ctx, const khp_moments* m);
khp_status khp_get_moments(khp_ctx* ctx, khp_moments* out);

#define KHP_MOMENTS_DEVICE (1u << 0)     /* every pointer is device memory of ctx's GPU */
typedef struct {
    float*    mean;       /* [H][W][3] or NULL */
    float*    m2;         /* [H][W][3] or NULL */
    uint32_t* count;      /* [H][W]    or NULL */
    uint32_t* bad;        /* [H][W]    or NULL */
    float*    rel_error;  /* [H][W]    or NULL */
} khp_moments_buffers;
khp_status khp_read_moments(khp_ctx* ctx, uint32_t flags, const khp_moments_buffers* out);
khp_status khp_moments_fold_host(uint32_t n_pixels, uint32_t first_sample, uint32_t n_samples,
                                 const float* samples, const khp_moments_buffers* state);   /* no device, no context */

/* ---- adaptive passes: render the unconverged pixels only -------------------------
 * khp_render_adaptive renders samples first_sample .. first_sample + spp - 1 for the
 * ACTIVE pixels of this rank only; the active pixels are chosen on the device from
 * the moments state (khp_set_moments must be on).
 *
 * Selection.  For an owned pixel with records a = (mean, n) and b = (m2, bad), let
 * t = n + bad.  The pixel is active iff
 *   first_sample == 0                      (a restart: every owned pixel; the fold's
 *                                           k == 0 rule zeroes the state), or
 *   t < min_samples, or
 *   (max_samples == 0 || t < max_samples) && (n < 2 || !(rel_error <= threshold)),
 * rel_error being the error plane's value (above) for a and b.  The comparison is
 * negated on purpose: a NaN error (an overflowed m2) stays active until max_samples
 * stops it, and so does a pixel below two finite samples, whose error is +inf by
 * definition, at every threshold, +inf included.  The active list is the owned list
 * (khp_gather_plan order) with the inactive pixels removed and the order kept: a
 * deterministic function of the arguments.  khp_adaptive_select_host is the same
 * rule, compiled from the same function, as a plain host loop: state holds the
 * planes mean, m2, count and bad by image pixel (rel_error is ignored), owned the
 * n_owned pixel indices, active has room for n_owned.  KHP_EINVAL: a null argument
 * (owned and active may be NULL when n_owned == 0), a null state plane, a bad
 * threshold or reserved.
 *
 * Pass.  Every active pixel traces the samples khp_render traces for that pixel and
 * those sample indices (same keys, rays, bounces), so a sample's colour is
 * khp_render's bit for bit.  A caller advances first_sample by spp per pass whichever
 * pixels were active; a pixel's sample set is the union of the passes it was active
 * in.  spp is added whole: a pixel may end above max_samples by less than spp.
 *
 * Fold.  Per active pixel, in increasing k, the moments fold above, unchanged; then
 * framebuffer[pixel] = mean, a plain store ((0, 0, 0) while n == 0).  The
 * framebuffer's (k + 1) running mean is not applied: it assumes every pixel has k
 * samples.  Inactive pixels keep their state and their framebuffer value bit for
 * bit.  In a series run adaptively from sample 0 the framebuffer therefore equals
 * mean on every owned pixel and is finite everywhere; khp_read_rgba8, khp_denoise
 * with colour == NULL and khp_gather_framebuffer work on it as they are.  A later
 * khp_render pass folds the framebuffer by the global k as always: the moments stay
 * exact, the framebuffer then holds that arithmetic's result.
 *
 * p is as for khp_render; flags is 0, KHP_RENDER_OUT_DEVICE or
 * KHP_RENDER_NO_READBACK.  The call is synchronous: it completes frames in flight
 * first, drops every piece of work rendered ahead for another call and leaves none
 * behind.  A new size makes the framebuffer and a zeroed state.  With no active pixel
 * nothing is traced or folded, the call is KHP_OK and out_rgb is still delivered.
 * res (or NULL) receives the rank's pixel count and the active list's length.
 * KHP_EINVAL (checked before the context is touched, khp_last_error names the
 * cause): a null ctx, p or a, threshold negative or NaN (+inf is allowed),
 * reserved != 0, spp == 0 or above 2^24, KHP_RENDER_ASYNC or KHP_RENDER_STATS, and
 * khp_render's own cases.  KHP_ENOTREADY: moments off, or no tree.
 * KHP_EUNSUPPORTED: the light-path variant enabled.  A refused call changes no byte
 * of the state or the framebuffer.  KIRK has no counterpart. */
typedef struct {
    float    threshold;    /* a pixel is converged when rel_error <= threshold; >= 0, not NaN (+inf allowed) */
    uint32_t min_samples;  /* a pixel with count + bad <  min_samples is always active */
    uint32_t max_samples;  /* a pixel with count + bad >= max_samples is never active; 0: no cap */
    uint32_t reserved;     /* 0 */
} khp_adaptive_params;     /* 16 bytes */
void       khp_adaptive_defaults(khp_adaptive_params* out);   /* 0.05, 8, 0: starting values, not a measured optimum */

typedef struct { uint64_t owned, active, reserved[2]; } khp_adaptive_result;   /* 32 bytes */

khp_status khp_render_adaptive(khp_ctx* ctx, const khp_render_params* p, const khp_adaptive_params* a,
                               khp_adaptive_result* res /* nullable */, float* out_rgb);
khp_status khp_adaptive_select_host(const khp_adaptive_params* a, uint32_t first_sample,
                                    const khp_moments_buffers* state, uint32_t n_owned, const uint32_t* owned,
                                    uint32_t* active, uint32_t* n_active);   /* no device, no context */
/* Test hooks.  khp_debug_adaptive_select runs exactly the selection kernels of
 * khp_render_adaptive over a caller's state (host planes of n_pixels pixels) and
 * owned list, in scratch of its own: nothing of the context changes.  Only
 * active[0 .. *n_active) is written.  KHP_EINVAL as for the host entry, and an owned
 * index >= n_pixels.  khp_debug_adaptive_list returns the last adaptive pass's active
 * list: *n its length, pixels (or NULL) room for that many (the pass's res->owned
 * bounds it), select_ms (or NULL) the device time of that pass's selection -- the
 * three launches and the count's copy, between two HIP events (0 when nothing is
 * owned).  KHP_ENOTREADY before the first adaptive pass. */
khp_status khp_debug_adaptive_select(khp_ctx* ctx, const khp_adaptive_params* a, uint32_t first_sample,
                                     uint32_t n_pixels, const khp_moments_buffers* state, uint32_t n_owned,
                                     const uint32_t* owned, uint32_t* active, uint32_t* n_active);
khp_status khp_debug_adaptive_list(khp_ctx* ctx, uint32_t* n, uint32_t* pixels, double* select_ms);

/* ABI 7: the light-path (bidirectional) variant of KIRK's GLSL path tracer,
 * lbb_construction.compute:195-403 builds light subpaths
 * (generatePrimaryLightRays / traceLightRays / shadeLightRays) and
 * pt_shade.compute:146-201 connects every camera hit to the vertices of one
 * randomly chosen subpath (sampling.is_bidirectional) instead of KIRK's
 * next-event estimate.  Per sample index k of a render, `light_paths`
 * subpaths per light are traced, each with up to `vertices` vertices (the
 * first on the light).  The exact rules, with the points where the GLSL is
 * undefined and this restatement decides, are in DESIGN.md §10.  KIRK's GLSL
 * marks the feature "experimental"; its estimator is not KIRK's CPU one, so
 * frames differ from khp_render without it (not a parity mode). */
typedef struct {
    uint32_t enabled;       /* 0: KIRK's next-event estimate (default)                          */
    uint32_t light_paths;   /* samples_per_light: subpaths per light and sample index, 1..65536  */
    uint32_t vertices;      /* bounces_per_path: vertices per subpath incl. the light's, 1..16   */
    float bias;             /* debug.bias: connection-ray origin offset along the normal         */
    float bounce_bias;      /* debug.bounce_bias: light-ray origin offset and vertex pull-back   */
    float min_pdf;          /* debug.min_pdf: a light vertex with pdf <= min_pdf ends its subpath */
    uint32_t image_plane;   /* also connect each sample's light vertices to its point on the
                               sensor (shadeBDPTImagePlane, pt_shade.compute:17-97):
                               0 off; 1 (default) the GLSL's target as written, record j's ray
                               origin + bias * its direction, i.e. the PREVIOUS vertex nudged
                               along the segment (pt_shade.compute:38-44 with
                               lbb_construction.compute:229-235, 391-395); 2 the vertex itself
                               pulled back by bounce_bias, like the hit connections (ABI 8)   */
} khp_bdpt_params;
void khp_bdpt_params_defaults(khp_bdpt_params* out);   /* off; 256 paths, 4 vertices, 1e-4 x 3, image plane on */
khp_status khp_set_bdpt(khp_ctx* ctx, const khp_bdpt_params* params);
khp_status khp_get_bdpt(khp_ctx* ctx, khp_bdpt_params* out);

/* ---- ABI 16: Marschner's TT and TRT fibre paths ------------------------------
 * MarschnerHairBSDF::localSample (Bsdf.cpp:465-769) holds three lobes: R (surface
 * reflection), TT (through the fibre) and TRT (one reflection inside it), the
 * last two as a state machine carried across bounces in Bounce::mat_flags.  KIRK
 * ships with the choice pinned to R (`int p = 0;`, :669), and so does a context
 * by default: with lobes == KHP_HAIR_LOBE_R every frame, texture and query is
 * what it was before ABI 16.  With other lobes enabled an unflagged hit on a
 * Marschner material draws one of the enabled lobes uniformly (draw 9 of the
 * bounce), TT / TRT refract into the fibre and the following one or two hits --
 * each a bounce of `depth`, as in traceRays -- finish the path.
 * d'Eon's TT / TRT stay unported.  Frames with TT or TRT have no CPU oracle.
 * khp_set_hair_lobes completes in-flight frames and needs no rebuild; lobes == 0,
 * bits above 7 or reserved != 0 are KHP_EINVAL.  The light-path variant traces
 * the R lobe only: enabling it with TT or TRT on, or the reverse, is
 * KHP_EUNSUPPORTED. */
#define KHP_HAIR_LOBE_R   1u
#define KHP_HAIR_LOBE_TT  2u
#define KHP_HAIR_LOBE_TRT 4u
typedef struct {
    uint32_t lobes;      /* KHP_HAIR_LOBE_* bits, at least one */
    uint32_t reserved;   /* 0 */
} khp_hair_lobes;
void khp_hair_lobes_defaults(khp_hair_lobes* out);   /* lobes = KHP_HAIR_LOBE_R */
khp_status khp_set_hair_lobes(khp_ctx* ctx, const khp_hair_lobes* lobes);
khp_status khp_get_hair_lobes(khp_ctx* ctx, khp_hair_lobes* out);

/* ---- a thin-lens camera: depth of field ---------------------------------------
 * KIRK::Camera holds m_focus_distance (11) and m_f_stop (1.8), derives m_aperture =
 * m_focal_length / m_f_stop and builds lens rays in Camera::transformToDof
 * (Common/Camera.cpp:39-51); only its Whitted tracer calls that (Simple_CPU_Raytracer.cpp:
 * 58-60, 238-249), the path tracer never does.  A context therefore starts with radius 0,
 * and with radius 0 every frame, texture, AOV plane and query is what it was before: the
 * camera ray is the pinhole ray and no new random number is drawn.  With radius > 0 every
 * camera ray of khp_render, khp_render_adaptive and khp_render_aov, on every schedule, is
 * the lens ray below, one float32 operation per step in the order written (csrc/lens.h,
 * compiled for the host and for gfx950: the same bits):
 *   (p, d)   the pinhole ray of the path: p = camera.position, d its normalised direction;
 *   u, v     draws 10 and 11 of bounce 0 of the path's key (unused before);
 *   disk     Shirley and Chiu's concentric map of (u, v): a = 2u - 1, b = 2v - 1; a == 0
 *            and b == 0 give (0, 0); |a| > |b| gives r = a, phi = (pi/4)(b/a); otherwise
 *            r = b, phi = pi/2 - (pi/4)(a/b); the point (r cos phi, r sin phi), times
 *            radius: (lx, ly).  Uniform over the disk, the distribution of KIRK's
 *            glm::diskRand(m_aperture * 3) (rejection from rand()), here a function of the key;
 *   focus    ft = focus_distance (KHP_LENS_FOCUS_KIRK, Camera.cpp:41 as written: the point
 *            lies at focus_distance along the pixel's own ray, so the surface in focus is a
 *            sphere about the camera), or focus_distance / dot(d, fwd) with fwd =
 *            normalize(cross(axis_y, axis_x)) (KHP_LENS_FOCUS_PLANE: a plane at right angles
 *            to the axis; where dot(d, fwd) is not > 0, ft = focus_distance); f = p + d * ft;
 *   ray      start = (p + axis_x * lx) + axis_y * ly (Camera.cpp:45), direction
 *            normalize(f - start) (KIRK's glm::normalize(ndir) discards its result; the Ray
 *            constructor normalises).
 * khp_set_lens completes in-flight frames (they finish with the lens they started with),
 * drops render-ahead work and needs no rebuild; the framebuffer and the moments are not
 * touched; khp_set_scene and khp_set_camera leave the lens alone.  KHP_EINVAL (checked
 * before the context is touched; khp_last_error names the cause): a null argument, radius
 * negative or not finite, focus_distance not finite or <= 0, an unknown focus, reserved !=
 * 0.  The light-path variant's image-plane stage assumes a pinhole sensor: radius > 0
 * while it is enabled, and enabling it while radius > 0, is KHP_EUNSUPPORTED.  A refused
 * call changes nothing.  Lens-on frames have no CPU oracle.
 * khp_reproject keeps its pinhole model: under a lens a pixel's depth plane is measured
 * from a point of the lens, not from camera.position, so its `locate` step is off by at
 * most radius. */
#define KHP_LENS_FOCUS_KIRK  0u
#define KHP_LENS_FOCUS_PLANE 1u
typedef struct {
    float radius;           /* offset 0: lens radius in scene units; 0: a pinhole (the default) */
    float focus_distance;   /* 4: finite, > 0 */
    uint32_t focus;         /* 8: KHP_LENS_FOCUS_* */
    uint32_t reserved;      /* 12: 0 */
} khp_lens;                 /* 16 bytes */
void       khp_lens_defaults(khp_lens* out);   /* 0 (off), 11 (Camera.h:116), KIRK, 0 */
/* radius = (focal_length / f_stop) * 3.0f: m_aperture, times diskRand's factor; focus KIRK.
 * KHP_EINVAL: out null; focal_length, f_stop or focus_distance not finite and > 0. */
khp_status khp_lens_from_kirk(float focal_length, float f_stop, float focus_distance, khp_lens* out);
khp_status khp_set_lens(khp_ctx* ctx, const khp_lens* lens);
khp_status khp_get_lens(khp_ctx* ctx, khp_lens* out);
/* The definition as a plain host loop (no device, no context): item i is the camera ray of
 * sample samples[i] of pixel pixels[i] (y * width + x) under `seed`, as khp_render makes
 * it; orig and dir take 3 floats per item.  lens NULL or radius 0: the pinhole rays.
 * KHP_EINVAL: a null camera or array, width 0, n outside [1, 2^20], a lens khp_set_lens
 * would refuse. */
khp_status khp_camera_rays_host(const khp_camera* camera, const khp_lens* lens, uint32_t width, uint32_t seed,
                                uint32_t n, const uint32_t* pixels, const uint32_t* samples, float* orig, float* dir);
/* Test hook in the style of the khp_debug_* queries: one thread per item runs the
 * renderer's own camera-ray function with the context's camera and lens, on scratch of
 * its own; nothing of the context is touched.  Needs a scene; otherwise as above. */
khp_status khp_debug_camera_rays(khp_ctx* ctx, uint32_t width, uint32_t seed, uint32_t n, const uint32_t* pixels,
                                 const uint32_t* samples, float* orig, float* dir);

/* ---- an energy-conserving fibre: BSDF kind 11 (additive) -----------
 * KIRK's two hair BSDFs are kept as written, with their faults, and
 * next-event estimation treats them as Lambert.  KHP_BSDF_CHIANG_HAIR is the near-field
 * fibre model of Chiang et al. 2016 beside them: four lobes (R, TT, TRT, residual),
 * importance sampled from the four draws a hit already has, and evaluated towards the
 * light with its true value.  A white fibre (sigma_a = 0) reflects and transmits all it
 * receives.  Cones only: a triangle with such a material is KHP_EINVAL (no axis, no
 * radius).  khp_material's fields are reused:
 *   ior          eta                      roughness    beta_m (clamped to [0.01, 1] at use)
 *   specular[0]  beta_n (clamped alike)   specular[1]  the cuticle tilt alpha, degrees
 *   specular[2]  reserved, 0              volume       sigma_a per fibre diameter
 *   diffuse      the colour of the albedo AOV and of KIRK's ambient term
 *   shader       KHP_SHADER_SIMPLE
 * A ray that leaves such a hit into the fibre starts beyond the fibre's far wall (the
 * model scatters from the whole fibre); nothing else of the shading changes.  Scenes
 * without the kind select the kernels they selected before and render the same bits.
 * KHP_EUNSUPPORTED, in either order and changing nothing: a kind-11 material together
 * with the light-path variant, or with hair lobes other than R.  No CPU oracle.
 * khp_hair_material fills *out from a fibre colour (Chiang's colour map gives sigma_a);
 * KHP_EINVAL: a null argument, color outside (0, 1], a beta outside [0.01, 1],
 * |alpha_deg| > 30, ior not finite and > 1. */
khp_status khp_hair_material(const float color[3], float beta_m, float beta_n, float alpha_deg, float ior,
                             khp_material* out);
/* The definition as plain host loops (no device, no context; csrc/hair_pb.h, compiled for
 * the host and for gfx950: the same bits).  Item i: materials[i] (kind 11), the hair frame
 * uvw[i] (U, V, W: 9 floats, V the axis), the normal, w_o (to the viewer) and w_i (to the
 * light), 3 floats each, any length.  f [n][3] is the BSDF's value.  The sampler takes the
 * draws u_l, u_n, u_0, u_1 ([n][4]) and gives the direction [n][3], its pdf [n], f [n][3]
 * and valid [n] (0: a zero axis, or no energy to scatter; f and pdf are then 0).
 * KHP_EINVAL: a null array, n outside [1, 2^20], a material of another kind. */
khp_status khp_hair_eval_host(uint32_t n, const khp_material* materials, const float* uvw, const float* normal,
                              const float* wo, const float* wi, float* f);
khp_status khp_hair_sample_host(uint32_t n, const khp_material* materials, const float* uvw, const float* normal,
                                const float* wo, const float* draws, float* out_dir, float* pdf, float* f,
                                int32_t* valid);

/* ---- an importance-sampled HDR environment light (additive) ---------
 * KIRK's background is found only by rays that happen to escape, its texels end at 255,
 * and no next-event ray is sent towards it.  khp_set_env_light gives the context a
 * latitude-longitude map of float32 radiance and a sampling table built from it on the
 * device; a context starts without one, and without one every frame, AOV plane and query
 * is what it was, from the same kernel instances.  rgb is [height][width][3]; row 0 is
 * the -y pole, column i spans the azimuths [i, i + 1) 2 pi / width + rotation measured from
 * +x towards +z.  The definition is csrc/env_light.h, compiled for the host and for
 * gfx950, the same bits; every float step is one float32 operation:
 *   table    per texel p = ((0.2126 r + 0.7152 g) + 0.0722 b) * k_sinf((j + 0.5)(pi / H)), m
 *            the largest p; weight = p > 0 ? max(1, (uint32)((p / m) * 2^19)) : 0;
 *            row_cdf[j] the exclusive prefix of row j (W + 1 words, the row's sum last),
 *            marginal the exclusive prefix of the row sums (H + 1 words, the total last).
 *   sample   U = min((uint32)(u * 2^24), 2^24 - 1) for each of the two draws; X = floor(U0 *
 *            total / 2^24) picks the row with marginal[j] <= X < marginal[j + 1], Y =
 *            floor(U1 * rowsum / 2^24) the column likewise; inside the texel fy = min(((float)
 *            (X - marginal[j]) + 0.5) / (float)rowsum, 1 - 2^-24), fx likewise with the
 *            texel's weight; theta = (j + fy)(pi / H), phi = (i + fx)(2 pi / W) + rotation,
 *            d = (sin theta cos phi, -cos theta, sin theta sin phi).  The sampler returns
 *            eval(d), so the two agree bit for bit; valid is pdf > 0.
 *   eval     n = normalize(d); theta = k_asinf(n.y) + pi/2, phi = k_atan2f(n.z, n.x) -
 *            rotation; j = (int)(theta / (pi / H)), i = (int)((t - floor(t)) * W) with t =
 *            phi / 2 pi, both clamped into the map; radiance = rgb[j][i] * scale (nearest
 *            texel: the density's own piecewise-constant shape); pdf = (((float)weight /
 *            (float)total) * (float)(W H)) / (2 pi^2 * sqrtf(n.x^2 + n.z^2)), 0 where the
 *            root is 0.  A zero or NaN direction has radiance 0 and pdf 0.
 * At a hit whose BSDF kind has a non-zero evaluateLight (Lambertian reflection and
 * transmission, Marschner, kind 11) and with nee = 1, the hit's one shadow ray goes to the
 * map with probability `select` (1 without lights), drawn by P_LIGHT_SEL, in a direction
 * drawn by P_LIGHT_0 / P_LIGHT_1; otherwise KIRK's light choice is made from the rescaled
 * draw and its term is divided by 1 - select.  An escaping ray adds the map's radiance
 * iff nee = 0, or it is a camera ray, or the previous hit was of another kind (glass,
 * mirror, glossy, d'Eon, transparent).  With the light on, env.color and env_map are not
 * read for an escaping ray; the ambient term stays.
 * khp_set_env_light copies the map and builds the table; it completes in-flight frames
 * (they finish with the light they started with), drops render-ahead work and needs no
 * rebuild; the framebuffer and the moments are not touched; khp_set_scene and
 * khp_set_camera leave the light alone.  width = height = 0 turns the light off (rgb is
 * not read).  KHP_EINVAL (checked before the context is touched; khp_last_error names the
 * cause, the first bad texel included): a null argument, width outside 1..4096, height
 * outside 1..2048, unknown flags, nee > 1, scale not finite and > 0, rotation not finite or
 * beyond 8192 radians either way, select outside (0, 1], reserved != 0, a texel that is
 * negative or not finite, a black map.  KHP_EUNSUPPORTED, in either order and changing
 * nothing: the light with the light-path variant, or with hair lobes other than R.
 * Frames with the light on have no CPU oracle. */
#define KHP_ENV_LIGHT_DEVICE (1u << 0)   /* rgb is device memory of ctx's GPU */
typedef struct {
    uint32_t width, height;  /* offset 0, 4: 0 x 0: off (the default) */
    uint32_t flags;          /* 8: KHP_ENV_LIGHT_* */
    uint32_t nee;            /* 12: 1 (default): next-event rays towards the map; 0: escaping rays only */
    float scale;             /* 16: radiance multiplier, finite, > 0 (default 1) */
    float rotation;          /* 20: radians about +y, finite (default 0) */
    float select;            /* 24: in (0, 1]: chance that a hit's one shadow ray goes to the map when
                                the scene also has lights (default 0.5); ignored without lights */
    uint32_t reserved;       /* 28: 0 */
    const float* rgb;        /* 32: [height][width][3]; row 0 is the -y pole, like every image of this ABI */
} khp_env_light;             /* 40 bytes */
void       khp_env_light_defaults(khp_env_light* out);
khp_status khp_set_env_light(khp_ctx* ctx, const khp_env_light* light);   /* copies the map, builds the table */
khp_status khp_get_env_light(khp_ctx* ctx, khp_env_light* out);           /* rgb comes back NULL */
/* The definition as plain host loops (no device, no context; a host map only).  Tables:
 * weight [H][W], row_cdf [H][W + 1], marginal [H + 1].  Sample: draws [n][2] give dir
 * [n][3], pdf [n], radiance [n][3], valid [n].  Eval: dir [n][3] (any length) gives
 * radiance [n][3] and pdf [n].  KHP_EINVAL: what khp_set_env_light refuses, a device map, a
 * null array, n outside [1, 2^20]. */
khp_status khp_env_light_tables_host(const khp_env_light* light, uint32_t* weight, uint32_t* row_cdf,
                                     uint64_t* marginal);
khp_status khp_env_light_sample_host(const khp_env_light* light, uint32_t n, const float* draws, float* dir,
                                     float* pdf, float* radiance, int32_t* valid);
khp_status khp_env_light_eval_host(const khp_env_light* light, uint32_t n, const float* dir, float* radiance,
                                   float* pdf);
/* Test hooks in the style of the khp_debug_* queries: the tables the context built on the
 * device, and the device functions the renderer calls, one thread per item (the sampler
 * over draws, the evaluation over dir_in), on scratch of their own.  KHP_ENOTREADY
 * without a light. */
khp_status khp_debug_env_light_tables(khp_ctx* ctx, uint32_t* weight, uint32_t* row_cdf, uint64_t* marginal);
khp_status khp_debug_env_light(khp_ctx* ctx, uint32_t n, const float* draws, const float* dir_in, float* s_dir,
                               float* s_pdf, float* s_radiance, int32_t* s_valid, float* e_radiance, float* e_pdf);

/* ---- kmath itself, op by op, on the host and on the device ------------
 * The numeric definitions of csrc/kmath.h are compiled twice, by the host compiler and for
 * gfx950, and every parity claim of this library rests on the two giving the same bits.
 * These two entries apply one op of csrc/kmath_ops.h to n items so that a test can hold
 * each compile to a truth and the two to one another.  Item i reads the three 64-bit words
 * in[3 i .. 3 i + 2] and writes the three words out[3 i .. 3 i + 2] (unused outputs are 0).
 * Nothing is converted at the boundary: subnormals, NaN payloads and signed zeros arrive as
 * given.  A scalar float32 / uint32 / int32 argument k is the low half of word k, a float64
 * / uint64 / int64 argument is word k; a float32 result is the low half of out word 0 (the
 * high half 0).  The algebra ops read six floats f0..f5 = the low and high halves of words
 * 0, 1, 2 in that order, and write one float per output word:
 *   DOT, CROSS, REFLECT, ANGLE   (a, b) = (f0 f1 f2), (f3 f4 f5) in the function's order
 *   NORMALIZE                    (f0 f1 f2)
 *   REFRACT                      I = (f0 f1 f2), N = (f3 f4 f5), eta = f5
 *   ROTATE_ROWVEC                d = (f0 f1 f2), angle = f3, axis = (f4 f5 f2)
 *   FACEFORWARD                  N = Nref = (f0 f1 f2), I = (f3 f4 f5)
 *   GMIN, GMAX (f0, f2), GCLAMP (f0, f2, f4): scalars, one per word
 * (seven- and nine-float argument lists share a float so that an item stays three words).
 * khp_kmath_host needs no device and no context.  khp_debug_kmath runs one item per thread
 * in the manner of the khp_debug_* queries, on scratch of its own; it needs no scene, and
 * leaves the framebuffer, the moments and khp_stats alone.  KHP_EINVAL, before anything is
 * launched: a null argument, an op outside [0, KHP_KMATH_OP_COUNT), n outside [1, 2^20]. */
typedef enum {
    /* IEEE primitives as kmath writes them */
    KHP_KMATH_MUL = 0,        /* a * b */
    KHP_KMATH_ADD = 1,        /* a + b */
    KHP_KMATH_DIV = 2,        /* a / b */
    KHP_KMATH_SQRT = 3,       /* sqrtf(a) */
    KHP_KMATH_RSQRT = 4,      /* 1.0f / sqrtf(a) */
    KHP_KMATH_MULADD = 5,     /* t = a * b; t + c: two roundings */
    KHP_KMATH_FLOOR = 6,      /* floorf(a) */
    KHP_KMATH_F2I = 7,        /* (int)a, in-range a */
    KHP_KMATH_F2U = 8,        /* (uint32_t)a, in-range a */
    KHP_KMATH_I2F = 9,        /* (float)(int) */
    KHP_KMATH_U2F = 10,       /* (float)(uint32_t) */
    KHP_KMATH_U642F = 11,     /* (float)(uint64_t) */
    KHP_KMATH_D2I2D = 12,     /* (double)(int64_t)d, in-range d */
    KHP_KMATH_DMUL = 13, KHP_KMATH_DADD = 14, KHP_KMATH_DDIV = 15,   /* double a * b, a + b, a / b */
    KHP_KMATH_UMULHI = 16,    /* the high 64 bits of a 64 x 64 product (env_light.h) */
    /* float functions */
    KHP_KMATH_LDEXPF = 17,    /* k_ldexpf(a, (int32)b) */
    KHP_KMATH_SINF = 18, KHP_KMATH_COSF = 19, KHP_KMATH_ATANF = 20,
    KHP_KMATH_ATAN2F = 21,    /* k_atan2f(y = a, x = b) */
    KHP_KMATH_ASINF = 22, KHP_KMATH_ACOSF = 23, KHP_KMATH_EXPF = 24, KHP_KMATH_SINHF = 25,
    KHP_KMATH_HYPOTF = 26, KHP_KMATH_LOGF_D = 27, KHP_KMATH_POWF_D = 28,
    /* double functions */
    KHP_KMATH_J0 = 29, KHP_KMATH_LOG_D = 30, KHP_KMATH_EXP_D = 31, KHP_KMATH_POW_D = 32,
    /* integers */
    KHP_KMATH_LOWBIAS32 = 33,
    KHP_KMATH_PATH_KEY = 34,  /* path_key(seed = a, pixel = b, sample = c) */
    KHP_KMATH_DRAW_U32 = 35,  /* draw_u32(key = a, dim = b) */
    KHP_KMATH_DRAW_U01 = 36,  /* draw_u01(key = a, dim = b) */
    /* algebra */
    KHP_KMATH_DOT = 37, KHP_KMATH_CROSS = 38, KHP_KMATH_NORMALIZE = 39, KHP_KMATH_REFLECT = 40,
    KHP_KMATH_REFRACT = 41, KHP_KMATH_ROTATE_ROWVEC = 42, KHP_KMATH_ANGLE = 43, KHP_KMATH_FACEFORWARD = 44,
    KHP_KMATH_GMIN = 45, KHP_KMATH_GMAX = 46, KHP_KMATH_GCLAMP = 47,
    KHP_KMATH_OP_COUNT = 48
} khp_kmath_op;
khp_status khp_kmath_host(uint32_t op, uint32_t n, const uint64_t* in, uint64_t* out);
khp_status khp_debug_kmath(khp_ctx* ctx, uint32_t op, uint32_t n, const uint64_t* in, uint64_t* out);

/* Completes every frame enqueued with KHP_RENDER_ASYNC (ABI 5).  A progressive
 * caller (KIRK's PathTracer::render loop) enqueues its passes and syncs before
 * reading the texture; passes accumulate in call order.  Any synchronous call
 * (render, read, gather, scene change) also completes in-flight frames first. */
khp_status khp_sync(khp_ctx* ctx);

/* khp_set_scene with the per-object arrays in device memory of ctx's GPU:
 *   device: tri_v, tri_n, tri_mat, tri_frame, tri_uv, cone_base_r0,
 *           cone_apex_r1, cone_mat, cone_model;
 *   host:   materials, lights, camera, env, cone_models (the matrix table,
 *           inverted on the host), textures and their texel data,
 *           material_textures -- a device pointer there is refused (EINVAL).
 * The objects are flattened on the device; the arrays are
 * read during the call only.  Not with KHP_CTX_HOST_BUILD. */
khp_status khp_set_scene_device(khp_ctx* ctx, const khp_scene* scene);

/* khp_gen_hairball followed by khp_fibers_to_cones, on the device: writes
 * n_strands * (verts - 1) cones (float4 base.xyz r0 / apex.xyz r1) into the
 * device arrays d_base_r0 / d_apex_r1; bit-identical to the host pair. */
khp_status khp_gen_hairball_device(khp_ctx* ctx, uint32_t n_strands, uint32_t verts, const float center[3],
                                   float ball_radius, float root_radius, uint32_t seed, float* d_base_r0,
                                   float* d_apex_r1);

/* khp_gen_hairball followed by khp_fibers_to_triangles, on the device, into
 * device arrays of n_strands*(verts-1)*2*res*res triangles (9 floats each). */
khp_status khp_gen_hairball_tris_device(khp_ctx* ctx, uint32_t n_strands, uint32_t verts, const float center[3],
                                        float ball_radius, float root_radius, uint32_t seed, uint32_t resolution,
                                        float* d_v, float* d_n, float* d_frame);

/* Device memory on ctx's GPU for the arrays above (plain hipMalloc / hipFree),
 * and a synchronous copy (to_device 1: host -> device, 0: device -> host). */
khp_status khp_device_alloc(khp_ctx* ctx, size_t bytes, void** out);
khp_status khp_device_free(khp_ctx* ctx, void* p);
khp_status khp_device_copy(khp_ctx* ctx, void* dst, const void* src, size_t bytes, int to_device);

/* Copy the device framebuffer (running mean, W*H*3) to host. */
khp_status khp_read_framebuffer(khp_ctx* ctx, float* out_rgb);

/* KIRK::Tonemapper parameters (Utils/Tonemapping.h:22-33; defaults in the
 * comments; khp_tonemap_defaults() fills them). */
typedef struct {
    float exposure;     /* m_exposure   0     (exposure factor 2^exposure) */
    float bias;         /* m_biasParam  0.85                               */
    float gamma;        /* m_gammaval   1                                  */
    float contrast;     /* m_contParam  0     (0: off)                     */
    float white, black; /* m_white 1, m_black 0                            */
    int32_t rec_gamma;  /* m_use_rec_gamma 0                               */
    int32_t center_weight;   /* m_center_weight 0: world luminance from a
                                Gaussian window (luminance_from_center)     */
    float kernel_multiplier; /* m_kernel_multiplier 0.125                   */
    int32_t center_x, center_y; /* m_center_x/y -1: W/2, H/2                */
} khp_tonemap;

/* Output stage on the device: PathTracer::drawTexture -> Texture::setPixel
 * (CPU_PathTracer.cpp:61-90, Texture.h:252-254), optionally after
 * PathTracer::applyToneMapping -> Tonemapper::map (CPU_PathTracer.cpp:92-104,
 * Tonemapping.cpp).  out_rgba: W*H*4 bytes, row y = KIRK texture row y (row 0
 * = bottom of the frame); byte = (uint8)max(min(c*255, 255), 0) truncated,
 * NaN -> 0; alpha 255.  tm = NULL: no tonemapping. */
khp_status khp_read_rgba8(khp_ctx* ctx, const khp_tonemap* tm, uint8_t* out_rgba);

/* ABI 8: the same 8-bit texture (tm = NULL form) without waiting, for a viewer
 * that shows every progressive pass (KIRK's GUI calls PathTracer::render once
 * per sample, CPU_PathTracer.cpp:17-52, then draws the texture).  The
 * conversion is enqueued in call order behind the asynchronous renders, like
 * a gather (inside a fused batch it runs between two frames' accumulates);
 * out_rgba (W*H*4 bytes of the frame it follows) is written by the time
 * khp_snapshot_wait(ticket) or khp_sync returns and must stay valid until
 * then.  Tonemapped textures need KIRK's sequential host sum and stay
 * synchronous (khp_read_rgba8). */
khp_status khp_read_rgba8_async(khp_ctx* ctx, uint8_t* out_rgba, uint64_t* ticket);
/* Delivers snapshot `ticket` and every older one.  wait = 1: enqueues what is
 * still pending and blocks; wait = 0: KHP_ENOTREADY if it has not completed. */
khp_status khp_snapshot_wait(khp_ctx* ctx, uint64_t ticket, int wait);

/* The Tonemapper member defaults (Tonemapping.h:23-33). */
void khp_tonemap_defaults(khp_tonemap* tm);

/* Batch forms of CPU_DataStructure::closestIntersection / isIntersection
 * (CPU_DataStructure.h:25-28, BVH impl CPU_BVH.cpp:51-93), on the GPU.
 * orig/dir: [n][3] host arrays; dir is normalised like KIRK::Ray (Ray.cpp:11-15).
 * closest: t_out = lambda (FLT_MAX if none), obj_out = object id or -1,
 *          uv_out (optional, [n][2]) = barycentric u,v (0 for cones).
 * any:     hit_out[i] = 1 if an object is hit with t in [0, tmax[i]]. */
khp_status khp_trace_closest(khp_ctx* ctx, uint32_t n, const float* orig, const float* dir,
                             float* t_out, int32_t* obj_out, float* uv_out);
khp_status khp_trace_any(khp_ctx* ctx, uint32_t n, const float* orig, const float* dir,
                         const float* tmax, uint8_t* hit_out);

khp_status khp_get_stats(khp_ctx* ctx, khp_stats* out);

/* ---- multi-GPU: tile sharding + RCCL framebuffer gather -------------------- */
/* RCCL unique id (128 bytes), created on rank 0 and broadcast by the caller. */
khp_status khp_comm_unique_id(uint8_t out_id[128]);
/* Joins the RCCL communicator of nranks ranks (one process per GPU).  ABI 11:
 * the communicator is non-blocking (ncclConfig_t.blocking = 0) and no call of
 * this context waits without a bound while it exists: RCCL calls are polled to
 * completion, and every device wait (khp_sync, synchronous renders, reads,
 * khp_destroy) polls ncclCommGetAsyncError.  An RCCL error, or an RCCL
 * operation that stays runnable (the work queued before it done) without
 * completing for the context's timeout (khp_comm_set_timeout, default 120 s:
 * e.g. a peer that never joins or a gather without its counterpart; a wait on
 * compute alone is never cut short, ABI 11 as amended in round 5), aborts the
 * communicator (ncclCommAbort) and returns KHP_EDEVICE with a message naming
 * this rank and its peers; gathers then return KHP_ENOTREADY until the next
 * khp_comm_init.  KIRK has no multi-device path; its only failure mode is the
 * loud exit of CPU_PathTracer.cpp:236-240. */
khp_status khp_comm_init(khp_ctx* ctx, int nranks, int rank, const uint8_t id[128]);
/* ABI 11: the bound (ms, > 0) of the waits above, for this context. */
khp_status khp_comm_set_timeout(khp_ctx* ctx, uint32_t timeout_ms);
/* Gather every rank's owned tiles (per p->tile_*) into rank root's device
 * framebuffer over RCCL; root may then khp_read_framebuffer. Collective. */
khp_status khp_gather_framebuffer(khp_ctx* ctx, const khp_render_params* p, int root);

/* ABI 8: an in-process group of contexts (rank = index in ctxs, all on one
 * device) for khp_gather_framebuffer without RCCL -- RCCL needs one GPU per
 * rank, this transport lets one process (e.g. a single-GPU test box) run every
 * rank's contexts and the product's gather plan, pack and unpack kernels.  A
 * sender's k-th gather packs into ring slot k % 64, stamped with k; the root's
 * k-th gather copies every sender's slot k, so each sender must have ENQUEUED
 * its k-th gather (khp_sync flushes fused frames) before the root's k-th gather
 * is enqueued (else the root's call returns KHP_ENOTREADY; a gather issued
 * with no asynchronous renders pending can then be repeated, but one queued
 * behind pending asynchronous renders runs when that fused batch is enqueued,
 * and its KHP_ENOTREADY then ends the batch where it stands: khp_sync the
 * senders before such a root gather), and a sender 64 gathers ahead of the root gets KHP_ENOTREADY instead of
 * overwriting a slot the root has not taken (ABI 11: stamps; before, both cases
 * copied stale pixels silently).  A member's pack into a slot waits for the
 * root's copy of its previous content.  Re-initialising a member removes it
 * from its old group. */
khp_status khp_comm_init_local(khp_ctx* const* ctxs, int nranks);

/* ABI 8: the pixel plan khp_gather_framebuffer moves, as seen from `rank`
 * (host only, no device needed).  KIRK has no multi-device path; its analogue
 * is the square-segment split of BufferSegmentation (Utils/BufferSegmentation.h:
 * 34-75).  Tile t (tile_size px, 0 -> 64, row-major) is rendered by rank
 * t % nranks.  counts (nullable, [nranks]): pixels rank r sends to root in
 * this rank's view -- the root lists every sender, a sender lists only itself,
 * the root's own entry is 0; pixels (nullable): their pixel indices y*W + x,
 * concatenated in rank order, each tile as 8x8 blocks; *n_pixels = the total.
 * A sender's counts[rank] equals the root's counts[rank] by construction. */
khp_status khp_gather_plan(uint32_t width, uint32_t height, uint32_t tile_size, int nranks, int rank, int root,
                           uint64_t* counts, uint32_t* pixels, uint64_t* n_pixels);

/* The BVH khp_build_accel built (device or host path), in the layout of
 * khp_host_build below: call with null arrays for *n_nodes / *depth. */
khp_status khp_read_bvh(khp_ctx* ctx, uint32_t* n_nodes, uint32_t* depth, float* node_boxes, int32_t* node_first,
                        int32_t* node_count, int32_t* object_ids);

/* The traversal records khp_build_accel left in HBM: n_records interior-node
 * records (64 B each: L.min.xyz L.max.x | L.max.yz R.min.xy | R.min.z R.max.xyz
 * | Lref Rref Lcnt Rcnt), n_slots primitive records (16 floats) and their aux
 * words (base_d, material, object, flags).  Null arrays: sizes only. */
khp_status khp_read_layout(khp_ctx* ctx, uint32_t* n_records, uint32_t* n_slots, void* node_records,
                           float* prim_records, uint32_t* prim_aux);

/* ---- host-only introspection (no device needed) ---------------------------- */
/* Runs exactly the flatten + BVH build of khp_set_scene/khp_build_accel on the
 * host.  Call with null arrays first to get *n_nodes / *depth.  Nodes are in
 * DFS preorder (node, left subtree, right subtree), like the recursion of
 * BVHNode::split (CPU_BVH.cpp:95-138).
 *   node_boxes [n_nodes][6] bmin.xyz bmax.xyz; node_first/node_count: leaf
 *   candidate range into object_ids (count 0 = interior, first = -1);
 *   object_ids [n_obj] leaf order; obj_bounds [n_obj][9] bmin bmax centroid;
 *   records [n_obj][16] the 64-byte intersection record of every object. */
khp_status khp_host_build(const khp_scene* scene, uint32_t* n_nodes, uint32_t* depth, float* node_boxes,
                          int32_t* node_first, int32_t* node_count, int32_t* object_ids, float* obj_bounds,
                          float* records);

/* ABI 12 (round 5): the host half of the tonemapped texture (khp_read_rgba8 with a
 * khp_tonemap): KIRK's `float sum; sum += log(...)` over the per-pixel log
 * luminances (Tonemapping.cpp:66-91, the terms in double, every step rounded
 * to float), continued from `start`, bit for bit but at one double add per
 * pixel (tonemap_host.cpp).  Exposed for tests and hosts that tonemap their own
 * framebuffer reads. */
khp_status khp_tonemap_log_sum(const double* terms, uint64_t n, float start, float* out);

/* Debug introspection: when the last synchronous khp_render ran with
 * khp_ctx_params.dump_bounce = b, the extension rays of bounce b (queue order) are
 * kept on the host.  Call with null arrays to get *n, then with [n][3] arrays. */
khp_status khp_debug_queue(khp_ctx* ctx, uint32_t* n, float* orig, float* dir);
/* The same render's shadow rays of bounce b as k_shadow traces them (after the
 * zero-colour skip): origin, direction ([n][3]) and t_max ([n]). */
khp_status khp_debug_shadow_queue(khp_ctx* ctx, uint32_t* n, float* orig, float* dir, float* tmax);
/* ---- ABI 15: batch queries of the shading functions (test hooks) ------------
 * Each runs the device functions the renderer calls on n independent items,
 * one thread per item, so a test can pin them item by item (a float64
 * reference, the oracle).  They add nothing to the render path.  All of them:
 * n in [1, 2^20], no null array, a built scene; every object / material /
 * light index is checked on the host -- KHP_EINVAL with khp_last_error naming
 * the first bad item -- and nothing is launched for a refused call.
 *
 * khp_debug_surface: the closest hit of ray i (origin, direction [n][3]; the
 * direction is normalised as KIRK::Ray does) and the surface there: t ([n],
 * FLT_MAX on a miss), object id (-1), the shading normal [n][3], the hair
 * frame U V W [n][9] (the cone's, or the fibre's for fur triangles; zero for
 * plain triangles and on a miss) and the material index (-1). */
khp_status khp_debug_surface(khp_ctx* ctx, uint32_t n, const float* orig, const float* dir, float* t,
                             int32_t* object, float* normal, float* uvw, int32_t* material);
/* BSDF::sample of material[i] (index into the scene's materials, untextured)
 * at a synthetic hit on object[i] (its hair frame), for ray_in in[i], normal
 * n[i], sample[i][2], the two hair draws hair[i][2] and the incoming flags.
 * kinds_mask selects the compiled instance: 0x7FF for KIRK's eleven kinds, or
 * (1 << LAMBERTIAN_REFLECTION) | (1 << MARSCHNER_HAIR), the set the renderer
 * compiles for fur-only scenes; (1 << 12) - 1 or (1 << LAMBERTIAN_REFLECTION) |
 * (1 << CHIANG_HAIR) for the instance with kind 11 compiled in (a kind-11 item
 * takes sample[i] as u_l, u_n and hair[i] as u_0, u_1, and has no early exit;
 * the two sets select the same instance); any other mask, or an item whose
 * material's kind is outside the mask, is KHP_EINVAL (the instance has that
 * case compiled out).  Outputs: direction [n][3], pdf [n], f [n][3], the sample
 * as written back [n][2], flags [n], valid [n] (0: the dot(in, n) == 0 early
 * exit).  Outputs the BSDF does not write are the inputs / 0. */
khp_status khp_debug_bsdf_sample(khp_ctx* ctx, uint32_t n, uint32_t kinds_mask, const int32_t* object,
                                 const int32_t* material, const float* in, const float* normal,
                                 const float* sample, const float* hair, const int32_t* flags_in, float* out_dir,
                                 float* pdf, float* f, float* sample_out, int32_t* flags_out, int32_t* valid);
/* ABI 16: MarschnerHairBSDF::localSample with the lobe set `lobes` (the argument,
 * not the context's setting) -- the device function the renderer calls when TT
 * or TRT is on -- for the same kind of item: lobe_u[i] is the lobe draw of an
 * unflagged first hit, hair[i][2] the alpha / beta draws, flags_in[i] the path's
 * flags (MATFLAG_CYLINDER_T_BOUNCE 8, _TR_BOUNCE 16 select the call of the state
 * machine).  Every material[i] must be KHP_BSDF_MARSCHNER_HAIR and `lobes` a
 * non-empty subset of 7, else KHP_EINVAL.  Outputs as khp_debug_bsdf_sample's;
 * the calls that only redirect the ray leave pdf and the sample at 0. */
khp_status khp_debug_hair_sample(khp_ctx* ctx, uint32_t n, uint32_t lobes, const int32_t* object,
                                 const int32_t* material, const float* in, const float* normal, const float* hair,
                                 const float* lobe_u, const int32_t* flags_in, float* out_dir, float* pdf, float* f,
                                 float* sample_out, int32_t* flags_out, int32_t* valid);
/* BSDF::evaluateLight for the same kind of item and the direction out[i]: f [n][3].
 * An item of kind 11 gives the fibre model's value f(w_o = out[i], w_i = in[i]). */
khp_status khp_debug_bsdf_eval(khp_ctx* ctx, uint32_t n, const int32_t* object, const int32_t* material,
                               const float* in, const float* normal, const float* out, float* f);
/* Light::calcLightdir (randomize = true) of light[i] from point[i] with the
 * draws draws[i][2]: the shadow ray's origin and direction [n][3] and the
 * attenuation [n]. */
khp_status khp_debug_light_dir(khp_ctx* ctx, uint32_t n, const int32_t* light, const float* point,
                               const float* draws, float* ray_orig, float* ray_dir, float* attenuation);
/* Light::isIntersection and sampleLightSource of light[i] for ray i: hit [n]
 * (0 / 1), t [n] (0 on a miss), the emitted colour [n][3]. */
khp_status khp_debug_light_isect(khp_ctx* ctx, uint32_t n, const int32_t* light, const float* orig,
                                 const float* dir, uint8_t* hit, float* t, float* emitted);
/* ---- ABI 17: queries of the light-path variant (test hooks) -----
 * Same rules as the ABI 15 queries: one item per thread, the device functions
 * the renderer calls, every index and count checked on the host (KHP_EINVAL,
 * nothing launched), scratch of their own -- no framebuffer, statistics, frame
 * in flight or render-ahead state is touched.  They use the context's current
 * khp_bdpt_params -- light_paths, vertices, bias, bounce_bias, min_pdf and
 * image_plane -- whether or not the variant is enabled.  A vertex record is 10
 * floats: valid (0 / 1), position, incoming direction, hit colour.
 *
 * khp_debug_light_paths: the renderer's light-subpath kernel itself for the one
 * sample index k and the render seed `seed`: out is
 * [light_paths][n_lights][vertices][10]; invalid vertices are all zero.
 * KHP_EINVAL for a scene without lights or when light_paths * n_lights *
 * vertices exceeds 2^20. */
khp_status khp_debug_light_paths(khp_ctx* ctx, uint32_t seed, uint32_t k, float* out);
/* One hit connection per item: the closest hit of the camera ray (orig, dir
 * [n][3], the direction normalised as KIRK::Ray does) and the surface there,
 * then the connection at bounce[i] (<= 4095) to vertex[i] (a record, its index
 * j[i] < 16) of a subpath of light[i].  Outputs: hit [n] (0: the camera ray
 * missed), accepted [n] (0: a miss or an invalid vertex; the rest of the item
 * is then zero), the connection ray's origin and direction [n][3], t_max [n]
 * and the contribution c_j [n][3].  No occlusion test. */
khp_status khp_debug_bdpt_connect(khp_ctx* ctx, uint32_t n, const float* orig, const float* dir,
                                  const uint32_t* bounce, const int32_t* light, const uint32_t* j,
                                  const float* vertex, uint8_t* hit, uint8_t* accepted, float* ray_orig,
                                  float* ray_dir, float* tmax, float* cj);
/* One image-plane connection per item in a width x height frame (both enter the
 * sensor area): from sensor[i] ([n][3]) to the target of record j[i] (< 16),
 * given records j - 1 (prev, ignored for j = 0) and j (cur), [n][10] each,
 * with the context's image_plane (1 or 2; 0 is KHP_EINVAL).  Outputs: accepted
 * [n] (0: an invalid vertex, the rest zero), the visibility ray's direction
 * [n][3], its length t [n] and the term c_j [n][3].  No occlusion test. */
khp_status khp_debug_img_connect(khp_ctx* ctx, uint32_t width, uint32_t height, uint32_t n, const float* sensor,
                                 const uint32_t* j, const float* prev, const float* cur, uint8_t* accepted,
                                 float* dir, float* t, float* cj);
/* ---- queries of the texture lookups (test hooks, additive) -------
 * Same rules as the ABI 15 queries: one item per thread, the device functions
 * the renderer calls, n in [1, 2^20], no null array, a built scene, every index
 * checked on the host (KHP_EINVAL naming the first bad item, nothing launched),
 * scratch of their own -- context, framebuffer and statistics untouched.
 *
 * khp_debug_tex_color: Texture::getColor of texture tex[i] (index into the
 * scene's textures) at xy[i] ([n][2]) -> rgba [n][4].  The textures are on the
 * device only for a scene with a textured material parameter or an environment
 * map; any other scene is KHP_EINVAL. */
khp_status khp_debug_tex_color(khp_ctx* ctx, uint32_t n, const int32_t* tex, const float* xy, float* rgba);
/* Environment::getColor for the direction dir[i] ([n][3], normalised as
 * KIRK does) -> rgb [n][3]. */
khp_status khp_debug_env_color(khp_ctx* ctx, uint32_t n, const float* dir, float* rgb);
/* The closest hit of ray i (as khp_debug_surface) and what the shader reads
 * there: t ([n], FLT_MAX on a miss), object id (-1), the hit's barycentrics
 * [n][2] (u, v; zero for cones), calcTcoord's texcoord [n][2], and the material
 * with its textured parameters resolved: diffuse, specular, volume, emission
 * ([n][3] each) and roughness [n].  A miss leaves all of these zero.  A scene
 * without textures is KHP_EINVAL (no triangle texcoords on the device). */
khp_status khp_debug_material(khp_ctx* ctx, uint32_t n, const float* orig, const float* dir, float* t,
                              int32_t* object, float* barycentrics, float* texcoord, float* diffuse,
                              float* specular, float* volume, float* emission, float* roughness);
/* ABI 13, test hook for the bounded device waits of a rank: builds
 * one RCCL-operation bracket (events `pre` / `post`, as around an ncclSend /
 * ncclRecv) on the context stream around a gate kernel that spins until
 * `release_ms` after the call starts (or 10 s), then waits for the stream with
 * the bound `bound_ms` as khp_sync would on a rank.  scenario 0: the gate
 * before `pre` (the operation never became runnable: no timeout); 1: the gate
 * between `pre` and `post` (runnable, not completing: KHP_EDEVICE after the
 * bound); 2: `pre` only, no `post` (retired once `pre` completes, then no
 * timeout).  *waited_ms: the wait's wall time.  The context keeps no
 * communicator state afterwards.  No RCCL call is made. */
khp_status khp_debug_comm_wait(khp_ctx* ctx, int scenario, uint32_t bound_ms, uint32_t release_ms,
                               double* waited_ms);

/* ---- registries / host helpers --------------------------------------------- */
/* BsdfFactory::getBsdf / ShaderFactory::getShader by KIRK name; -1 if unknown
 * (KIRK throws std::invalid_argument, BsdfFactory.cpp:39-45). */
int khp_bsdf_kind_from_name(const char* name);
const char* khp_bsdf_name(int kind);
int khp_shader_kind_from_name(const char* name);

/* Camera::applyParameters (Camera.cpp:6-37) for a camera at `position`
 * looking along `look_at` (a direction, KIRK m_local_look_at) with `up`;
 * sensor size and focal length in metres (KIRK defaults 0.036x0.024, 0.0415). */
khp_status khp_camera_setup(const float position[3], const float look_at[3], const float up[3],
                            float sensor_w, float sensor_h, float focal_length,
                            uint32_t width, uint32_t height, khp_camera* out);

/* ABI 13: replaces the scene's camera without rebuilding anything (KIRK's GUI
 * moves the Camera between PathTracer::render calls and resets the pass
 * count, after which render() restarts its buffers, CPU_PathTracer.cpp:17-19).
 * Completes in-flight frames first; the next render uses the new camera.
 * Drops render-ahead work. */
khp_status khp_set_camera(khp_ctx* ctx, const khp_camera* camera);

/* Moved geometry without a rebuild (still ABI 17: symbols only).  khp_update_geometry
 * re-flattens the objects of `moved` and refits the tree khp_build_accel left in HBM: the
 * topology (children, leaf ranges, object order, slots, references) stays, every box,
 * primitive record and base_d is recomputed, the two-level and top-of-tree records are
 * remade.  Box union is min / max, so the refitted tree has one right answer per bit (up
 * to the sign of a zero); khp_refit_host below computes the same on the host.
 *
 * Read from `moved`: n_tris, tri_v, tri_n, tri_frame, n_cones, cone_base_r0, cone_apex_r1.
 * Materials, material indices, lights, camera, environment, textures, tri_uv, cone_models
 * and cone_model stay as khp_set_scene left them.  khp_update_geometry_device takes the
 * five arrays in device memory, as khp_set_scene_device does.
 *
 * KHP_EINVAL with the context unchanged: a null argument, n_tris or n_cones other than
 * the built scene's, a missing array.  KHP_ENOTREADY: no tree yet.  KHP_EUNSUPPORTED: a
 * KHP_CTX_HOST_BUILD context (its tree is not in HBM).  A NaN, an infinity or a float32
 * overflow in the moved coordinates is KHP_EINVAL with khp_set_scene's messages, found
 * after the object arrays were overwritten: the context is then left un-built
 * (khp_render returns KHP_ENOTREADY) until the next successful khp_update_geometry, or
 * khp_set_scene + khp_build_accel.  KHP_EDEVICE if a refitted box is not the union of
 * its children's (never, for a tree this library built); that, or any other device error
 * once the object arrays have started to change, leaves the context un-built in the same way.
 *
 * Like khp_set_camera the call completes frames in flight first and drops render-ahead
 * work and parked paths of the old geometry.  The running mean, the sample counts and
 * the moments are the caller's to restart: render the next frame with first_sample = 0.
 *
 * sah_cost = (sum over interior nodes of A(n) + sum over leaves of count(n) A(n)) / A(root),
 * A the surface area of the float32 box evaluated in double: what the refit's looser
 * boxes cost, next to sah_cost_built of the tree as khp_build_accel left it. */
typedef struct {
    double   refit_ms;        /* wall time of the call, transfers included                    */
    double   kernel_ms;       /* HIP-event time of its kernels (three intervals, summed)      */
    double   sah_cost;        /* of the tree as it now stands                                 */
    double   sah_cost_built;  /* of the tree as khp_build_accel left it                       */
    uint32_t n_updates;       /* successful updates since the last khp_build_accel            */
    uint32_t reserved;
    float    root_box[6];
} khp_refit_info;

khp_status khp_update_geometry(khp_ctx* ctx, const khp_scene* moved, khp_refit_info* info /* may be NULL */);
khp_status khp_update_geometry_device(khp_ctx* ctx, const khp_scene* moved, khp_refit_info* info);
/* The info of the last successful update; before the first one sah_cost == sah_cost_built,
 * n_updates == 0 and the times are 0.  KHP_ENOTREADY without a tree, KHP_EUNSUPPORTED on a
 * KHP_CTX_HOST_BUILD context. */
khp_status khp_get_refit_info(khp_ctx* ctx, khp_refit_info* out);
/* Host-only twin of the device refit (no device needed): flattens `moved` as khp_host_build
 * does (a whole scene here: its materials and tables are checked as khp_set_scene checks
 * them), then refits a topology given as khp_read_bvh / khp_host_build return it (preorder,
 * count == 0 = interior, object_ids in leaf order).  node_boxes [n_nodes][6], obj_bounds
 * [n_obj][9], records [n_obj][16] and sah_cost are outputs, each nullable.  KHP_EINVAL
 * with nothing written: a null input, counts that do not describe a preorder tree of
 * n_nodes nodes over the scene's objects, an object id out of range. */
khp_status khp_refit_host(const khp_scene* moved, uint32_t n_nodes, const int32_t* node_first,
                          const int32_t* node_count, const int32_t* object_ids,
                          float* node_boxes, float* obj_bounds, float* records, double* sah_cost);

/* Which compile-time instance of a render kernel a launch takes (still ABI 17: symbols
 * only; csrc/variant.h).  No device and no context: the renderer's own
 * selectors and tables, for tests and tools.  An instance is returned as its template
 * arguments in declaration order, defaults filled in, a bool as 0 / 1:
 *   KHP_KERNEL_PATH          tex, wide, kinds, ra, qs, lens, env
 *   KHP_KERNEL_SHADE         tex, bd, kinds, lens, env
 *   KHP_KERNEL_EXTEND        stats, cam, wide, top, lens
 *   KHP_KERNEL_SHADOW        stats, wide, top
 *   KHP_KERNEL_AOV_TRACE     tex, lens
 *   KHP_KERNEL_GENERATE      lens
 *   KHP_KERNEL_SHADOW_FINISH bd
 * args holds at least 7 words; n_args receives the count. */
typedef enum {
    KHP_KERNEL_PATH = 0,
    KHP_KERNEL_SHADE = 1,
    KHP_KERNEL_EXTEND = 2,
    KHP_KERNEL_SHADOW = 3,
    KHP_KERNEL_AOV_TRACE = 4,
    KHP_KERNEL_GENERATE = 5,
    KHP_KERNEL_SHADOW_FINISH = 6,
    KHP_KERNEL_COUNT = 7
} khp_kernel_family;
/* Flags (0 / nonzero), but `bounce`.  The first seven are a batch's facts; the others are
 * the inputs of one launch, each read by the families named. */
typedef struct {
    uint32_t textured;     /* the scene has textured materials or an environment map        */
    uint32_t fur_only;     /* its materials use Lambert reflection and Marschner hair only   */
    uint32_t lobes_on;     /* khp_set_hair_lobes: a lobe set other than R                    */
    uint32_t hair;         /* a KHP_BSDF_CHIANG_HAIR material                                */
    uint32_t env;          /* khp_set_env_light: the light is on                             */
    uint32_t lens_on;      /* khp_set_lens: radius > 0                                       */
    uint32_t bd;           /* khp_set_bdpt: the light-path variant runs                      */
    uint32_t bounce;       /* shade: the bounce shaded                                       */
    uint32_t cam0;         /* shade: bounce 0 recomputes its camera rays                     */
    uint32_t stats;        /* extend, shadow: an instrumented render                         */
    uint32_t cam;          /* extend: the launch makes its camera rays in place              */
    uint32_t wide;         /* path, extend, shadow: on the two-level records                 */
    uint32_t top;          /* extend, shadow: khp_ctx_params.lds_nodes                       */
    uint32_t has_top;      /* extend, shadow: the tree has top records                       */
    uint32_t ahead;        /* path: render-ahead is on                                       */
    uint32_t queue_start;  /* path: the launch starts from a bounce's queue (path_from)      */
} khp_variant_facts;
/* The instance launched for `facts`, whether or not a setter would refuse the combination.
 * grid_kind (nullable) receives 1 where a shade launch takes the light-path instances' grid,
 * else 0.  KHP_EINVAL: a null argument, an unknown family. */
khp_status khp_kernel_variant_host(uint32_t kernel, const khp_variant_facts* facts, uint32_t* args,
                                   uint32_t* n_args, uint32_t* grid_kind);
/* Row `index` of the family's table of compiled instances.  KHP_EINVAL: a null argument,
 * an unknown family, an index past the table's end. */
khp_status khp_kernel_variant_table(uint32_t kernel, uint32_t index, uint32_t* args, uint32_t* n_args);

/* Fur fibers -> cone frusta exactly as CPU_Scene::flattenNode does with
 * m_fiberAsCylinder (CPU_Scene.cpp:121-144): base pulled back by 0.8 % of the
 * segment, base radius shrunk 5 % (segment index <= 3) or 10 %.
 * positions [n_fibers][verts][3], radii [n_fibers][verts];
 * out arrays [n_fibers*(verts-1)][4]. */
khp_status khp_fibers_to_cones(uint32_t n_fibers, uint32_t verts_per_fiber,
                               const float* positions, const float* radii,
                               float* out_base_r0, float* out_apex_r1);

/* Fur fibers -> triangle tubes exactly as CPU_Scene::fiberToTriangles
 * (CPU_Scene.cpp:232-345, identity mesh transform), the flatten path KIRK
 * takes with m_fiberAsCylinder = false: per segment a (res+1)^2 vertex grid
 * and 2 res^2 triangles, each carrying the segment's frame.
 * out_v / out_n / out_frame: [n_fibers*(verts-1)*2*res*res][3][3]. */
khp_status khp_fibers_to_triangles(uint32_t n_fibers, uint32_t verts_per_fiber, const float* positions,
                                   const float* radii, uint32_t resolution, float* out_v, float* out_n,
                                   float* out_frame);

/* Seeded synthetic inputs (stand-ins for SceneGraph + Mesh::addFurToFaces,
 * Mesh.cpp:82-148).  Bit-reproducible on any host.
 * hairball: roots uniform on a sphere, strands of `verts` vertices following
 * the addFurToFaces recurrence in the root's tangent frame.
 * positions [n][verts][3], radii [n][verts]. */
khp_status khp_gen_hairball(uint32_t n_strands, uint32_t verts, const float center[3],
                            float ball_radius, float root_radius, uint32_t seed,
                            float* positions, float* radii);
/* ---- ABI 14: fur on an arbitrary triangle mesh ------------------------------
 * Replaces Mesh::addFurToFaces (Common/Mesh.cpp:82-148), which
 * SceneGraph::addFurFibersToAllMeshes(5, 10, 0.004) runs on every mesh
 * (Demo/main.cpp:235): per face, fibres rooted at uniform points of the
 * triangle, each following the recurrence of Mesh.cpp:114-142.
 *
 * Every fibre draws from its own key, a function of (seed, face index, fibre
 * index within the face) only: a face's fur does not change when another
 * face's count or shape does.  Root (Mesh.cpp:104-112): two draws r1, r2,
 * mirrored (1 - r1, 1 - r2) when r1 + r2 >= 1, root = (a + r1 (b - a)) +
 * r2 (c - a).  KIRK draws from [0, 1], the key's draws lie in [0, 1): a
 * difference of measure zero.  KIRK seeds from std::random_device; here the
 * result is a function of `seed`, bit for bit on host and device. */
#define KHP_FUR_FRAME_KIRK   0  /* Mesh.cpp as written: lift along +y, lean along +z of the mesh's own space */
#define KHP_FUR_FRAME_NORMAL 1  /* the same recurrence in the root's tangent frame (as the seeded hairball):
                                   local y = shading normal at the root, local z = lean direction */
typedef struct {
    uint32_t fibers_per_face;  /* KIRK's count (Demo: 5); used when density == 0, at most 65,535 */
    float    density;          /* > 0: fibres per unit area instead.  A face of area A = 0.5 |(b-a) x (c-a)|
                                  gets floor(A * density + u) fibres, u a draw of the face's own key
                                  (stochastic rounding: small faces keep their share); a NaN area gives 0 */
    uint32_t verts;            /* vertices per fibre, 2..64 (Demo: 10) */
    float    root_radius;      /* > 0 (Demo: 0.004); KIRK refuses <= 0, Mesh.cpp:85-89 */
    float    scale;            /* > 0; multiplies KIRK's metre constants (0.003 sink, ln(i)/90 lift, 0.06 lean,
                                  0.001 tip radius); 1 = KIRK's.  x * 1.0f is exact, so 1 changes no bit */
    uint32_t frame;            /* KHP_FUR_FRAME_* */
    float    comb[3];          /* FRAME_NORMAL only: lean direction before projection into the tangent plane
                                  (used when the projection is at least 1e-6 long); (0,0,0) = a seeded random
                                  tangent per fibre, as the hairball does */
    uint32_t seed;
    uint32_t reserved;         /* 0 */
} khp_fur_params;              /* 44 bytes */
/* Fills the Demo's call: 5, 0, 10, 0.004, 1, KIRK, 0 0 0, 0x4B49524B. */
void khp_fur_params_defaults(khp_fur_params* out);

/* FRAME_NORMAL: the normal at the root is normalize((1-r1-r2) na + r1 nb + r2 nc); when
 * that sum is shorter than 1e-6 or not finite, the geometric normal
 * normalize((b-a) x (c-a)), and (0,1,0) when that fails too.
 *
 * All three calls return KHP_EINVAL when root_radius <= 0, scale <= 0, verts is
 * outside 2..64, frame is unknown, density is negative or not finite, a face's
 * count would reach 65,536 (the message names the face), or the cones
 * n_fibers * (verts - 1) exceed UINT32_MAX - n_tris (a scene's object ids are
 * 32 bits).  fibers_per_face == 0 with density == 0 is a valid empty result.
 *
 * Host only: the number of fibres, and (face_first nullable, [n_tris + 1]) the
 * exclusive prefix of the per-face counts; face f owns fibres
 * [face_first[f], face_first[f+1]).  tri_v as khp_scene.tri_v (read in density
 * mode only). */
khp_status khp_fur_count(const khp_fur_params* p, uint32_t n_tris, const float* tri_v, uint64_t* n_fibers,
                         uint32_t* face_first);
/* The fibres: positions [n_fibers][verts][3], radii [n_fibers][verts], face-major,
 * the fibre index within the face minor.  They feed khp_fibers_to_cones /
 * khp_fibers_to_triangles unchanged.  tri_n (as khp_scene.tri_n) is read with
 * FRAME_NORMAL only.  The fur is in the mesh's own space: a node transform goes
 * through khp_scene.cone_models. */
khp_status khp_gen_fur(const khp_fur_params* p, uint32_t n_tris, const float* tri_v, const float* tri_n,
                       float* positions, float* radii);
/* khp_gen_fur followed by khp_fibers_to_cones, on the device: d_tri_v / d_tri_n
 * and the outputs are device arrays of ctx's GPU; writes *n_cones = n_fibers *
 * (verts - 1) cones (float4 base.xyz r0 / apex.xyz r1), bit-identical to the
 * host pair and usable as khp_scene.cone_base_r0 / cone_apex_r1 of
 * khp_set_scene_device.  d_base_r0 == NULL: *n_cones only.  capacity_cones
 * (the cones the arrays hold) smaller than the count: KHP_EINVAL, nothing
 * written. */
khp_status khp_gen_fur_device(khp_ctx* ctx, const khp_fur_params* p, uint32_t n_tris, const float* d_tri_v,
                              const float* d_tri_n, uint64_t capacity_cones, float* d_base_r0, float* d_apex_r1,
                              uint64_t* n_cones);

/* icosphere with `subdiv` subdivisions: 20*4^subdiv triangles (tri_v/tri_n as khp_scene). */
khp_status khp_gen_icosphere(uint32_t subdiv, const float center[3], float radius,
                             float* tri_v, float* tri_n);
/* torus grid nu x nv quads -> 2*nu*nv triangles. */
khp_status khp_gen_torus(uint32_t nu, uint32_t nv, const float center[3], float major_r,
                         float minor_r, float* tri_v, float* tri_n);

#ifdef __cplusplus
}
#endif

#endif /* KIRK_HIP_H */
