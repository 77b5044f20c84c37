// rt_capi.cpp -- C ABI of libmi355rt.so (include/mi355rt.h): scene handles, render contexts, launches.
//
// Host side of the HIP path.  No CPU fallback: every render entry point fails with RT_ERR_NO_DEVICE /
// RT_ERR_DEVICE when there is no usable GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "mi355rt.h"
#include "rt_launch.h"       // every launcher of the kernel files, and struct Kernels
#include "rt_scene_dev.h"
#include "rt_scene_image.hpp" // the scene image (blob, light tables, FrameArgs' scene words): shared with the test tools
#include "rt_frame_host.hpp"  // camera tables, per-frame camera words, halo rows: shared with the test tools
#include "rt_set_scene.h"
#include "scene-exception.h"
#include "scene.h"
#include "camera.h"

// the launchers a context calls per floating-point contraction mode (rt_launch.h, struct Kernels); rt_create picks one from RT_FLAG_FAST
// Every slot is filled by its name: the seven queries' launchers have one type on all three paths, so a list by position would compile with two of them swapped.
#define RT_KERNELS(V)                                                                               \
    [] {                                                                                            \
        Kernels k{};                                                                                \
        k.trace = RT_CAT(rt_launch_trace, V);                                                       \
        k.wavefront = RT_CAT(rt_launch_wavefront, V);                                               \
        k.stream = RT_CAT(rt_launch_stream, V);                                                     \
        k.stream_cull = RT_CAT(rt_launch_stream_cull, V);                                           \
        k.stream_cull_bounce = RT_CAT(rt_launch_stream_cull_bounce, V);                             \
        k.ray_list = RT_CAT(rt_launch_ray_list, V);                                                 \
        k.stream_ray_list = RT_CAT(rt_launch_stream_ray_list, V);                                   \
        k.stream_cull_ray_list = RT_CAT(rt_launch_stream_cull_ray_list, V);                         \
        k.primary_rays = RT_CAT(rt_launch_primary_rays, V);                                         \
        k.query[PATH_STAGED].gbuffer = RT_CAT(rt_launch_gbuffer, V);                                \
        k.query[PATH_STAGED].pick = RT_CAT(rt_launch_pick, V);                                      \
        k.query[PATH_STAGED].object_extents = RT_CAT(rt_launch_object_extents, V);                  \
        k.query[PATH_STAGED].trace_rays = RT_CAT(rt_launch_trace_rays, V);                          \
        k.query[PATH_STAGED].occluded_rays = RT_CAT(rt_launch_occluded_rays, V);                    \
        k.query[PATH_STAGED].shade_rays = RT_CAT(rt_launch_shade_rays, V);                          \
        k.query[PATH_STAGED].trace_paths = RT_CAT(rt_launch_trace_paths, V);                        \
        k.query[PATH_STREAMED].gbuffer = RT_CAT(rt_launch_stream_gbuffer, V);                       \
        k.query[PATH_STREAMED].pick = RT_CAT(rt_launch_stream_pick, V);                             \
        k.query[PATH_STREAMED].object_extents = RT_CAT(rt_launch_stream_object_extents, V);         \
        k.query[PATH_STREAMED].trace_rays = RT_CAT(rt_launch_stream_trace_rays, V);                 \
        k.query[PATH_STREAMED].occluded_rays = RT_CAT(rt_launch_stream_occluded_rays, V);           \
        k.query[PATH_STREAMED].shade_rays = RT_CAT(rt_launch_stream_shade_rays, V);                 \
        k.query[PATH_STREAMED].trace_paths = RT_CAT(rt_launch_stream_trace_paths, V);               \
        k.query[PATH_CULLED].gbuffer = RT_CAT(rt_launch_pixel_cull_gbuffer, V);                     \
        k.query[PATH_CULLED].pick = RT_CAT(rt_launch_pixel_cull_pick, V);                           \
        k.query[PATH_CULLED].object_extents = RT_CAT(rt_launch_pixel_cull_object_extents, V);       \
        k.query[PATH_CULLED].trace_rays = RT_CAT(rt_launch_stream_cull_trace_rays, V);              \
        k.query[PATH_CULLED].occluded_rays = RT_CAT(rt_launch_stream_cull_occluded_rays, V);        \
        k.query[PATH_CULLED].shade_rays = RT_CAT(rt_launch_stream_cull_shade_rays, V);              \
        k.query[PATH_CULLED].trace_paths = RT_CAT(rt_launch_stream_cull_trace_paths, V);            \
        return k;                                                                                   \
    }()
static const Kernels kernels_strict = RT_KERNELS(strict), kernels_fast = RT_KERNELS(fast);
// ... and the launchers of a groups context (RT_FLAG_STREAM_CULL_GROUPS; rt_launch.h, struct GroupLaunchers), in a record of their own
#define RT_GROUP_LAUNCHERS(V)                                     \
    [] {                                                          \
        GroupLaunchers k{};                                       \
        k.frame = RT_CAT(rt_launch_stream_cull_groups, V);        \
        return k;                                                 \
    }()
static const GroupLaunchers group_launchers_strict = RT_GROUP_LAUNCHERS(strict), group_launchers_fast = RT_GROUP_LAUNCHERS(fast);

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// a failed HIP call is RT_ERR_DEVICE, named `what` in the message ("hipMalloc(scene) failed: ...") or by its own text
#define RT_TRY(what, call)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return fail(RT_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString(e_));       \
    } while (0)
#define RT_HIP(call) RT_TRY(#call, call)

// What a context owns on the device, one wrapper per kind: released when the context is deleted (rt_destroy makes the context's device
// current first).  They convert to the raw handle, so the code that uses them reads like code on raw pointers.
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};
template <typename T>
struct DevMem : NoCopy { // device memory
    T *p = nullptr;
    ~DevMem() { reset(); }
    void reset() { if (p) (void) hipFree(p); p = nullptr; }
    hipError_t alloc(size_t bytes) { reset(); return hipMalloc((void **) &p, bytes); }
    operator T *() const { return p; }
};
struct MappedWords : NoCopy { // host memory the device writes through a mapping
    uint32_t *p = nullptr;
    ~MappedWords() { reset(); }
    void reset() { if (p) (void) hipHostFree(p); p = nullptr; }
    operator uint32_t *() const { return p; }
};
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void) hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

// the staging buffers of an entry point that takes host arrays: an input and an output array that only grow, n elements each
struct Staging {
    DevMem<void> in, out;
    uint32_t cap = 0;
    int reserve(uint32_t n, size_t in_each, size_t out_each)
    {
        if (n <= cap) return RT_OK; // (every earlier call has synchronised: nothing uses the old buffers)
        in.reset();
        out.reset();
        cap = 0;
        const uint32_t want = n < 64u ? 64u : n;
        RT_HIP(in.alloc(in_each * (size_t) want));
        RT_HIP(out.alloc(out_each * (size_t) want));
        cap = want;
        return RT_OK;
    }
};

// one device buffer that only grows: the staging memory of the path entry points that take host arrays, laid out per call
struct Scratch {
    DevMem<unsigned char> p;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return RT_OK; // (every earlier call has synchronised: nothing uses the old buffer)
        p.reset();
        cap = 0;
        RT_HIP(p.alloc(bytes));
        cap = bytes;
        return RT_OK;
    }
};

// the C ABI's exception boundary of the scene entry points: a SceneException is RT_ERR_SCENE, anything else `other`
template <typename F>
int guarded(int other, F &&body)
{
    try {
        return body();
    } catch (const SceneException &e) {
        return fail(RT_ERR_SCENE, "%s", e.what());
    } catch (const std::bad_alloc &) {
        return fail(RT_ERR_NOMEM, "out of memory");
    } catch (const std::exception &e) {
        return fail(other, "%s", e.what());
    }
}

} // namespace

// Flat arrays the descriptor points into, kept next to the C++ scene model.
struct rt_scene {
    Scene scene;
    std::vector<double> coefs, light_p;
    std::vector<float> reflection, albedo, light_color;
    std::vector<uint8_t> light_kind;

    void flatten()
    {
        const size_t no = scene.objects.size(), nl = scene.lights.size();
        coefs.resize(no * RT_NCOEF);
        reflection.resize(no);
        albedo.resize(no * 3);
        for (size_t i = 0; i < no; i++) {
            const Object &o = scene.objects[i];
            std::memcpy(&coefs[i * RT_NCOEF], o.surface.data(), sizeof(double) * RT_NCOEF);
            reflection[i] = o.reflection_ratio;
            albedo[3 * i + 0] = o.color.x;
            albedo[3 * i + 1] = o.color.y;
            albedo[3 * i + 2] = o.color.z;
        }
        light_p.resize(nl * 3);
        light_color.resize(nl * 3);
        light_kind.resize(nl);
        for (size_t i = 0; i < nl; i++) {
            const LightSource &l = scene.lights[i];
            light_kind[i] = l.is_spherical ? 1 : 0;
            for (int k = 0; k < 3; k++) {
                light_p[3 * i + k] = l.p[k];
                light_color[3 * i + k] = l.light_color[k];
            }
        }
    }
};

// What culls whole chunks of the unit-sphere table, by family: each has a decision of its own (create_scene), work words of its own, and a getter and
// a debug reader in the ABI.  `also`: what else the work words need, as rt_debug_<name> says it when the context keeps none.
enum CullFamily {
    CULL_FRAME,    // rt_render (rt_stream_cull.hip; RT_FLAG_STREAM_CULL)
    CULL_BOUNCE,   // ... its bounce rays per ray as well (rt_stream_cull_bounce.hip; RT_FLAG_STREAM_CULL_BOUNCE)
    CULL_ADAPTIVE, // the halo and refine passes of an adaptive frame (rt_stream_cull_adaptive.hip)
    CULL_RAYS,     // caller-supplied rays, per ray (rt_stream_cull_rays.hip; RT_FLAG_STREAM_CULL_RAYS): four entry points share the words
    CULL_PIXELS,   // the pixel queries, by the block's cone (rt_stream_cull_pixels.hip; RT_FLAG_STREAM_CULL_PIXELS): three entry points share the words
    N_CULL_FAMILIES
};
static const char STATS_SET[] = " and MI355RT_STREAM_CULL_STATS=1 was set at rt_create";
static const struct {
    const char *get, *debug, *also;
} cull_family[N_CULL_FAMILIES] = {
    {"rt_get_stream_cull", "rt_debug_stream_cull", STATS_SET},
    {"rt_get_stream_cull_bounce", "rt_debug_stream_cull_bounce", STATS_SET},
    // (the kernel that counts for both classes is not built: rt_stream_cull_adaptive.hip)
    {"rt_get_stream_cull_adaptive", "rt_debug_stream_cull_adaptive",
     ", MI355RT_STREAM_CULL_STATS=1 was set at rt_create and the scene does not hold both general quadrics and degree-3 objects"},
    {"rt_get_stream_cull_rays", "rt_debug_stream_cull_rays", STATS_SET},
    {"rt_get_stream_cull_pixels", "rt_debug_stream_cull_pixels", STATS_SET},
};

struct rt_ctx {
    int device = 0;
    const Kernels *kern = &kernels_strict; // RT_FLAG_FAST: &kernels_fast
    rt_config cfg{};   // as the caller passed it (defaults filled in): the OUTPUT frame's bands and format
    FrameArgs fa{};    // what the render kernels draw: the output frame, or with supersampling the internal k x finer RGBA32F frame
    // output frame (what every entry point but the render kernels sees; the same as fa's geometry without supersampling)
    uint32_t width = 0, height = 0;
    uint32_t local_rows = 0, max_local_rows = 0;
    size_t pixel_bytes = 16;
    uint32_t ssaa = 1;          // samples per axis k (RT_FLAG_SSAA2 / RT_FLAG_SSAA4)
    DevMem<void> d_ss;          // k > 1: the internal frame's local rows, [k * local_rows][k * width] float4
    int resolve_nt = 0;         // the resolve reads the internal frame with non-temporal loads (MI355RT_RESOLVE_NT, experiments)
    // RT_FLAG_SSAA_ADAPTIVE (rt_adaptive.hip): fa is the output geometry (as for k = 1); k = ssaa samples per axis where a pixel is refined
    bool adaptive = false;
    float tau = 1.0f / 32.0f;   // rt_set_ssaa_threshold
    DevMem<void> d_p;           // RGBA8 output: the plain frame P, [local_rows][width] float4 (RGBA32F renders P in place)
    DevMem<void> d_halo;        // world > 1: [halo_slots][width] float4, slot 2b / 2b + 1 = the global row just below / above local band b
    uint32_t halo_slots = 0;
    uint64_t halo_rays = 0;     // centre rays the halo pass traces per frame (slots inside the image x width)
    DevMem<uint32_t> d_list;    // [local_rows * width] refined pixels, (local row << 16) | x; d_list[local_rows * width] = their count
    DevMem<double> d_camxk, d_camyk;      // camera-plane tables of the k-times finer sample grid
    uint32_t ray_grid = 0, halo_grid = 0; // workgroups of the ray-list kernel (fixed per context)
    // RT_FLAG_SSAA_GEOMETRY: the primary-hit planes of this rank's rows and the halo rows' records
    bool geometry = false;
    float min_cos = -INFINITY;   // rt_set_ssaa_geometry; -inf: object ids only, the normal plane is not formed
    DevMem<int32_t> d_geo_obj;   // [local_rows][width]
    DevMem<float> d_geo_nrm;     // [local_rows][width] float4
    DevMem<uint32_t> d_geo_xy;   // world > 1: [halo_slots * width][2] global coordinates of the halo rows' pixels (constant)
    DevMem<void> d_geo_halo;     // world > 1: [halo_slots][width] rt_hit
    DevMem<DevObject> d_obj;     // the scene blob (rt_scene_dev.h)
    DevMem<DevLight> d_light;    // [DevLight x n_lights][LightK x n_lights]
    DevMem<void> d_fb;
    DevMem<unsigned long long> d_counters;
    Event ev0, ev1;  // the pair behind `ms` of every timed entry point (a context belongs to one thread at a time, and a timed call has waited for ev1 when it returns)
    Event ev_done;   // recorded behind every render: a render on ANOTHER stream waits for it (frames of a context are ordered)

    hipStream_t last_stream = nullptr;
    bool rendered = false;
    bool captured = false;      // the last render was recorded into a stream capture: ev_done was not (an event recorded inside a capture orders nothing outside it)
    bool counted = false;
    bool zero_counters = false; // diagnostic builds: clear counters[] before every render
    DevMem<uint64_t> d_stamps;
    DevMem<double> d_camx, d_camy; // per-column / per-row camera-plane coordinates
    size_t n_stamp_rows = 0;
    uint64_t frame = 0; // renders so far: selects the launch-order generation (FrameArgs::order_state); 64 bits: frame % 3 must never skip
    uint32_t tag = 0;   // frame tag of the scan workgroups' tile words (FrameArgs::tile_state); unique per render, never 0
    DevMem<uint32_t> d_order, d_tiles; // what FrameArgs::order_state / tile_state point at
    MappedWords h_listed;         // host-mapped words the kernel writes (FrameArgs::ord_host)
    uint32_t ord_split = 0;       // FrameArgs::ord_split of non-sparse frames
    std::vector<double> cub_coefs; // the 20 coefficients of the first RT_CUB_AT_MAX degree-3 objects (FrameArgs::cub_at is formed from them every frame)
    bool stream_queries = false;  // the queries are the streamed kernels (rt_stream_queries.hip): RT_FLAG_STREAM_QUERIES on a streamed context or on a scene whose tables the staged query kernels cannot hold in LDS
    bool stream_adaptive = false; // the halo, G and refine passes of an adaptive frame are the streamed kernels (rt_stream_adaptive.hip, rt_stream_queries.hip): RT_FLAG_STREAM_ADAPTIVE on a scene or context the staged passes refuse
    bool streamed = false;        // rt_render is the streamed frame kernel (rt_stream.hip): RT_FLAG_STREAM, or a scene whose tables the context's own kernel cannot hold in LDS
    // Chunk culling, per family (CullFamily): the decision (create_scene) and what its launchers take -- the bounds of the 64-entry chunks of the (ordered)
    // unit-sphere table, and the family's 8 of d_cull_words (NULL where it keeps none: create_device_state); all zero where the family does not cull
    bool cull[N_CULL_FAMILIES] = {};
    ChunkTables chunks[N_CULL_FAMILIES] = {};
    uint32_t n_chunks = 0;
    DevMem<UsEntry> d_bounds;
    DevMem<unsigned long long> d_cull_words; // [N_CULL_FAMILIES][8]; only with MI355RT_STREAM_CULL_STATS=1 in the environment at rt_create
    // rt_reorder_scene (rt_reorder_scene.hip): the decision (create_scene; RT_FLAG_STREAM_CULL_REORDER on a context whose frame culls), its work space (sized
    // from n_us alone) and the workgroups a launch of it may take (MI355RT_REORDER_MAX_GRID at rt_create lowers it: the tests reach the grids' second trip with it)
    bool reorder = false;
    DevMem<unsigned char> d_reorder_work;
    uint32_t reorder_max_grid = 0;
    // A second level over those bounds (RT_FLAG_STREAM_CULL_GROUPS; rt_stream_cull_groups.hip): the decision (create_scene), one bound per 64 chunk bounds, the
    // launchers of the variant, and 8 work words of its own (only with MI355RT_STREAM_CULL_STATS=1 at rt_create)
    bool words_wanted = false; // MI355RT_STREAM_CULL_STATS=1 was in the environment at rt_create (read once, in create_scene)
    bool groups = false;
    uint32_t n_groups = 0;
    DevMem<UsEntry> d_groups;
    DevMem<unsigned long long> d_group_words;
    GroupTables group_tables = {};
    const GroupLaunchers *group_kern = &group_launchers_strict; // RT_FLAG_FAST: &group_launchers_fast
    // the launchers of the pixel and the ray entry points: the staged, the streamed (stream_queries) or the culled (cull[CULL_PIXELS], cull[CULL_RAYS]) path of kern->query
    const QueryLaunchers *pixel_q = nullptr, *ray_q = nullptr;
    bool lean_ok = false;         // the scene qualifies for the wave-per-block instantiation (FrameArgs::lean; dense frames only)
    bool lean_now = true;         // ... and it renders the current frames (it does not while few tiles have hits: see choose_schedule)
    uint32_t wg_slots = 1536;     // workgroup slots of the device for these kernels (six per CU)
    int lean_force = 0;           // MI355RT_LEAN=always / never (experiments)
    bool ord_on = true;           // launch-order feedback in use (off while most tiles have hits)
    Staging pick;  // rt_pick: [cap][2] coordinates in, [cap] rt_hit out; created on first use
    Staging ext;   // rt_object_extents_host: [cap] rt_object_extent out (nothing goes in); created on first use
    Staging rq;    // the _host ray entry points: [cap] rt_ray in, [cap] rt_hit out (rt_shade_rays_host: its 4 x float32 pixels); created on first use
    Scratch pth;   // rt_trace_paths_host / rt_pick_paths: [rays][max_segments planes][last][ends][coordinates]; created on first use
    // scene updates (rt_set_scene): the kernel's status block, and the staging memory of rt_set_scene_host, created on first use
    DevMem<SetSceneStatus> d_ss_status;
    DevMem<unsigned char> d_ss_stage;
};

// ---------------------------------------------------------------------------------------------------
#ifdef RT_DIAGNOSTIC_BUILD
extern "C" int rt_abi_version(void) { return RT_ABI_VERSION | RT_ABI_DIAGNOSTIC; } // stamps / experiment exits / spills allowed: not the product
#else
extern "C" int rt_abi_version(void) { return RT_ABI_VERSION; }
#endif

extern "C" const char *rt_last_error(void) { return g_last_error.c_str(); }

extern "C" void rt_set_last_error(const char *message) { g_last_error = message ? message : ""; }

// ---- scene --------------------------------------------------------------------------------------------
// a new scene handle around `make()`'s Scene
template <typename F>
static int scene_handle(rt_scene **out, F &&make)
{
    std::unique_ptr<rt_scene> s(new rt_scene());
    s->scene = make();
    s->flatten();
    *out = s.release();
    return RT_OK;
}

extern "C" int rt_scene_load_file(const char *path, rt_scene **out)
{
    if (!path || !out) return fail(RT_ERR_INVALID, "rt_scene_load_file: null argument");
    *out = nullptr;
    return guarded(RT_ERR_SCENE, [&]() -> int { return scene_handle(out, [&] { return Scene::load_from_file(path); }); });
}

extern "C" int rt_scene_new(uint32_t width, uint32_t height, double fov_deg, uint32_t max_reflections,
                            const float bg_color[3], rt_scene **out)
{
    if (!out || !bg_color) return fail(RT_ERR_INVALID, "rt_scene_new: null argument");
    *out = nullptr;
    return guarded(RT_ERR_NOMEM, [&]() -> int {
        return scene_handle(out, [&] { return Scene(width, height, fov_deg, max_reflections, glm::vec3(bg_color[0], bg_color[1], bg_color[2])); });
    });
}

extern "C" int rt_scene_add_object(rt_scene *s, const double coefs[RT_NCOEF], float reflection_ratio, const float color[3])
{
    if (!s || !coefs || !color) return fail(RT_ERR_INVALID, "rt_scene_add_object: null argument");
    return guarded(RT_ERR_NOMEM, [&]() -> int {
        SurfaceCoefs sc{};
        std::memcpy(sc.data(), coefs, sizeof(double) * RT_NCOEF);
        s->scene.objects.push_back(Object(sc, reflection_ratio, glm::vec3(color[0], color[1], color[2])));
        s->flatten();
        return RT_OK;
    });
}

extern "C" int rt_scene_add_light(rt_scene *s, int is_spherical, float intensity, const double v[3], const float color[3])
{
    if (!s || !v || !color) return fail(RT_ERR_INVALID, "rt_scene_add_light: null argument");
    return guarded(RT_ERR_NOMEM, [&]() -> int {
        const glm::dvec3 dv(v[0], v[1], v[2]);
        const glm::vec3 c(color[0], color[1], color[2]);
        s->scene.lights.push_back(is_spherical ? LightSource::spherical(intensity, dv, c) : LightSource::directional(intensity, dv, c));
        s->flatten();
        return RT_OK;
    });
}

extern "C" int rt_surface_make(int kind, const double a[3], const double b[3], double out_coefs[RT_NCOEF])
{
    if (!out_coefs) return fail(RT_ERR_INVALID, "rt_surface_make: null output");
    if ((kind <= 2 && !a) || (kind <= 1 && !b)) return fail(RT_ERR_INVALID, "rt_surface_make: null argument");
    return guarded(RT_ERR_NOMEM, [&]() -> int {
        SurfaceCoefs sc{};
        switch (kind) {
        case 0: sc = SurfaceCoefs::sphere(glm::dvec3(a[0], a[1], a[2]), b[0]); break;
        case 1: sc = SurfaceCoefs::plane(glm::dvec3(a[0], a[1], a[2]), glm::dvec3(b[0], b[1], b[2])); break;
        case 2: sc = SurfaceCoefs::dingDong(glm::dvec3(a[0], a[1], a[2])); break;
        case 3: sc = SurfaceCoefs::clebsch(); break;
        case 4: sc = SurfaceCoefs::cayley(); break;
        default: return fail(RT_ERR_INVALID, "rt_surface_make: unknown kind %d", kind);
        }
        std::memcpy(out_coefs, sc.data(), sizeof(double) * RT_NCOEF);
        return RT_OK;
    });
}

extern "C" int rt_scene_set_size(rt_scene *s, uint32_t width, uint32_t height)
{
    if (!s) return fail(RT_ERR_INVALID, "rt_scene_set_size: null scene");
    s->scene.px_width = width;
    s->scene.px_height = height;
    return RT_OK;
}

extern "C" int rt_scene_set_max_reflections(rt_scene *s, uint32_t max_reflections)
{
    if (!s) return fail(RT_ERR_INVALID, "rt_scene_set_max_reflections: null scene");
    s->scene.max_reflections = max_reflections;
    return RT_OK;
}

extern "C" int rt_scene_get_desc(const rt_scene *s, rt_scene_desc *out)
{
    if (!s || !out) return fail(RT_ERR_INVALID, "rt_scene_get_desc: null argument");
    std::memset(out, 0, sizeof(*out));
    out->width = s->scene.px_width;
    out->height = s->scene.px_height;
    out->vertical_fov = s->scene.vertical_fov;
    out->bg_color[0] = s->scene.bg_color.x;
    out->bg_color[1] = s->scene.bg_color.y;
    out->bg_color[2] = s->scene.bg_color.z;
    out->max_reflections = s->scene.max_reflections;
    out->n_objects = (uint32_t) s->scene.objects.size();
    out->n_lights = (uint32_t) s->scene.lights.size();
    out->coefs = s->coefs.data();
    out->reflection = s->reflection.data();
    out->albedo = s->albedo.data();
    out->light_is_spherical = s->light_kind.data();
    out->light_p = s->light_p.data();
    out->light_color = s->light_color.data();
    return RT_OK;
}

extern "C" void rt_scene_free(rt_scene *s) { delete s; }

extern "C" int rt_camera_matrix(const double pos[3], double yaw_deg, double pitch_deg, double out_cam[16])
{
    if (!pos || !out_cam) return fail(RT_ERR_INVALID, "rt_camera_matrix: null argument");
    Camera c;
    c.position = glm::dvec3(pos[0], pos[1], pos[2]);
    c.yaw = yaw_deg;
    c.pitch = pitch_deg;
    const glm::dmat4 m = c.matrix();
    for (int col = 0; col < 4; col++)
        for (int row = 0; row < 4; row++) out_cam[col * 4 + row] = m[col][row];
    return RT_OK;
}

// ---- render -------------------------------------------------------------------------------------------
static uint32_t rows_of_rank(uint32_t height, uint32_t band, uint32_t world, uint32_t rank)
{
    // bands b = rank, rank + world, ... ; the last band of the image may be partial
    uint32_t n_bands = (height + band - 1) / band, rows = 0;
    for (uint32_t b = rank; b < n_bands; b += world) {
        uint32_t y0 = b * band;
        rows += (y0 + band <= height) ? band : height - y0;
    }
    return rows;
}

// MI355RT_DEBUG_FRAME0 / MI355RT_DEBUG_TAG0 (tests: a context that starts late in its life, just in front of a counter's restart):
// an unsigned number, decimal or 0x hex, nothing behind it, at most `max`.  Unset: *value is left alone.
static int debug_start_value(const char *name, uint64_t max, uint64_t *value)
{
    const char *e = std::getenv(name);
    if (!e) return RT_OK;
    const bool hex = e[0] == '0' && (e[1] == 'x' || e[1] == 'X');
    const char *p = hex ? e + 2 : e;
    uint64_t v = 0;
    bool ok = *p != '\0';
    for (; ok && *p; p++) {
        const int c = (unsigned char) *p;
        const int d = (c >= '0' && c <= '9') ? c - '0' : ((hex && c >= 'a' && c <= 'f') ? c - 'a' + 10 : ((hex && c >= 'A' && c <= 'F') ? c - 'A' + 10 : -1));
        const uint64_t base = hex ? 16u : 10u;
        ok = d >= 0 && v <= (UINT64_MAX - (uint64_t) d) / base;
        if (ok) v = v * base + (uint64_t) d;
    }
    if (!ok) return fail(RT_ERR_INVALID, "rt_create: %s=\"%s\" is not an unsigned decimal or 0x hexadecimal number", name, e);
    if (v > max) return fail(RT_ERR_INVALID, "rt_create: %s=%s exceeds 0x%llX", name, e, (unsigned long long) max);
    *value = v;
    return RT_OK;
}

// ---- rt_create, step by step ------------------------------------------------------------------------------
// a table the context keeps on the device: hipMalloc, then hipMemcpy from src or, without one, hipMemset to zero
template <typename T>
static int device_table(DevMem<T> &d, const void *src, size_t bytes, const char *what)
{
    hipError_t e = d.alloc(bytes);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "hipMalloc(%s) failed: %s", what, hipGetErrorString(e));
    e = src ? hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) : hipMemset(d, 0, bytes);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "%s(%s) failed: %s", src ? "hipMemcpy" : "hipMemset", what, hipGetErrorString(e));
    return RT_OK;
}

// 1. everything that can be refused without a device, in this order (a machine without a GPU sees the same refusals)
static int create_checks(rt_ctx *ctx, const rt_scene_desc *sd, const rt_config *cfg_in)
{
    rt_config &cfg = ctx->cfg;
    cfg.device = -1;
    cfg.world = 1;
    if (cfg_in) cfg = *cfg_in;
    if (cfg.world == 0) cfg.world = 1;
    if (cfg.band_rows == 0) cfg.band_rows = 8;
    if (cfg.rank >= cfg.world) return fail(RT_ERR_INVALID, "rt_create: rank %u >= world %u", cfg.rank, cfg.world);
    if (cfg.format > RT_FMT_RGBA8) return fail(RT_ERR_INVALID, "rt_create: unknown format %u", cfg.format);
    if ((cfg.flags & RT_FLAG_SSAA2) && (cfg.flags & RT_FLAG_SSAA4))
        return fail(RT_ERR_INVALID, "rt_create: RT_FLAG_SSAA2 and RT_FLAG_SSAA4 exclude each other");
    const uint32_t k = ctx->ssaa = (cfg.flags & RT_FLAG_SSAA4) ? 4u : ((cfg.flags & RT_FLAG_SSAA2) ? 2u : 1u);
    ctx->adaptive = (cfg.flags & RT_FLAG_SSAA_ADAPTIVE) != 0;
    if (ctx->adaptive && k == 1u) return fail(RT_ERR_INVALID, "rt_create: RT_FLAG_SSAA_ADAPTIVE needs RT_FLAG_SSAA2 or RT_FLAG_SSAA4");
    ctx->geometry = (cfg.flags & RT_FLAG_SSAA_GEOMETRY) != 0;
    if (ctx->geometry && !ctx->adaptive) return fail(RT_ERR_INVALID, "rt_create: RT_FLAG_SSAA_GEOMETRY needs RT_FLAG_SSAA_ADAPTIVE");
    if ((cfg.flags & RT_FLAG_STREAM) && (cfg.flags & RT_FLAG_SIMPLE)) return fail(RT_ERR_INVALID, "rt_create: RT_FLAG_STREAM and RT_FLAG_SIMPLE exclude each other");
    if ((cfg.flags & RT_FLAG_STREAM_ADAPTIVE) && !ctx->adaptive) return fail(RT_ERR_INVALID, "rt_create: RT_FLAG_STREAM_ADAPTIVE needs RT_FLAG_SSAA_ADAPTIVE");
    if ((cfg.flags & RT_FLAG_STREAM) && ctx->adaptive && !(cfg.flags & RT_FLAG_STREAM_ADAPTIVE))
        return fail(RT_ERR_INVALID, "rt_create: RT_FLAG_STREAM is not available with RT_FLAG_SSAA_ADAPTIVE (the refine pass has no streamed kernel)");
    if ((cfg.flags & RT_FLAG_STREAM) && (cfg.flags & RT_FLAG_COUNT))
        return fail(RT_ERR_INVALID, "rt_create: RT_FLAG_STREAM is not available with RT_FLAG_COUNT (the streamed kernel books no counters)");
    if (sd->width == 0 || sd->height == 0) return fail(RT_ERR_INVALID, "rt_create: empty image %ux%u", sd->width, sd->height);
    if (k > 1u && ((uint64_t) k * sd->width > 65536u || (uint64_t) k * sd->height > 65536u))
        return fail(RT_ERR_INVALID, "rt_create: %ux%u supersampled %ux%u exceeds 65536 samples per axis", sd->width, sd->height, k, k);
    if ((sd->n_objects && (!sd->coefs || !sd->reflection || !sd->albedo)) ||
        (sd->n_lights && (!sd->light_is_spherical || !sd->light_p || !sd->light_color)))
        return fail(RT_ERR_INVALID, "rt_create: null scene array");
    // (tests) the frame number and the tile-word tag the context starts from; the device state starts zeroed whatever they say: tile words
    // with tag 0 never equal a live tag and all three launch-order generations are empty, so any starting frame % 3 is consistent
    uint64_t tag0 = 0;
    if (int rc = debug_start_value("MI355RT_DEBUG_FRAME0", UINT64_MAX, &ctx->frame)) return rc;
    if (int rc = debug_start_value("MI355RT_DEBUG_TAG0", 0x1FFFFFF0u, &tag0)) return rc;
    ctx->tag = (uint32_t) tag0;
    return RT_OK;
}

// 2. the context's own words and the geometry of the frame the kernels render (host only)
static void create_frame(rt_ctx *ctx, const rt_scene_desc *sd, int device)
{
    const rt_config &cfg = ctx->cfg;
    ctx->device = device;
    ctx->kern = (cfg.flags & RT_FLAG_FAST) ? &kernels_fast : &kernels_strict;
    ctx->group_kern = (cfg.flags & RT_FLAG_FAST) ? &group_launchers_fast : &group_launchers_strict;
    ctx->width = sd->width;
    ctx->height = sd->height;
    if (const char *e = std::getenv("MI355RT_RESOLVE_NT")) ctx->resolve_nt = std::atoi(e) != 0; // (experiments)
    ctx->pixel_bytes = cfg.format == RT_FMT_RGBA8 ? 4 : 16;
    ctx->local_rows = rows_of_rank(sd->height, cfg.band_rows, cfg.world, cfg.rank);
    for (uint32_t r = 0; r < cfg.world; r++) {
        uint32_t n = rows_of_rank(sd->height, cfg.band_rows, cfg.world, r);
        if (n > ctx->max_local_rows) ctx->max_local_rows = n;
    }

    // the frame the kernels render: with supersampling the unmodified scene at k times the size, into RGBA32F (k is a power of two, so
    // the aspect ratio is the same double; bands of k * band_rows rows keep each output row's samples with the rank that owns it)
    // (adaptive: the plain pass renders the output frame itself, k = 1 geometry; the sample rays come from the tables of create_adaptive)
    const uint32_t kf = ctx->adaptive ? 1u : ctx->ssaa;
    const uint32_t rw = kf * sd->width, rh = kf * sd->height;
    FrameArgs &fa = ctx->fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.aspect = (double) rw / rh;                      // Scene::aspect_ratio, include/scene.h:32-33
    fa.tan_half_fov = std::tan(0.5 * sd->vertical_fov); // init_update, src/update-cpu.cpp:28
    fa.bg[0] = sd->bg_color[0];
    fa.bg[1] = sd->bg_color[1];
    fa.bg[2] = sd->bg_color[2];
    fa.bg[3] = 1.0f;
    fa.width = rw;
    fa.height = rh;
    fa.max_refl = sd->max_reflections;
    fa.rank = cfg.rank;
    fa.world = cfg.world;
    fa.band_rows = kf * cfg.band_rows;
    fa.local_rows = kf * ctx->local_rows; // (= rows_of_rank(rh, k * band_rows, world, rank))
    fa.tiles_x = (rw + RT_TILE - 1) / RT_TILE;
    fa.n_tiles = fa.tiles_x * ((fa.local_rows + RT_TILE - 1) / RT_TILE);
    fa.rgba8 = (ctx->ssaa == 1u && cfg.format == RT_FMT_RGBA8) ? 1u : 0u; // (adaptive: P is RGBA32F)
    fa.ord_plain = (cfg.flags & RT_FLAG_PLAIN_ORDER) ? 1u : 0u;
    ctx->ord_split = (cfg.flags & RT_FLAG_NOSPLIT) ? 0u : RT_ORD_SPLIT_CLASSES;
    if (const char *e = std::getenv("MI355RT_SPLIT_CLASSES")) ctx->ord_split = (uint32_t) std::atoi(e) & 15u; // (experiments)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->wg_slots = 6u * (uint32_t) cus;
    if (const char *e = std::getenv("MI355RT_LEAN")) ctx->lean_force = (e[0] == 'a') ? 1 : ((e[0] == 'n') ? -1 : 0);
}

// 3. the scene image (rt_scene_image.hpp) and what it means for this context: the schedule it may take, the LDS it needs
static int create_scene(rt_ctx *ctx, const rt_scene_desc *sd, rtp::SceneImage &im)
{
    FrameArgs &fa = ctx->fa;
    im = rtp::scene_image(*sd, ctx->cfg.flags, fa);
    ctx->cub_coefs = im.cub_coefs;
    ctx->lean_ok = im.lean_ok && !std::getenv("MI355RT_NOLEAN"); // (experiments)
    // Which kernel is rt_render?  The streamed one (rt_stream.hip) where the caller asks for it, and where the context's own kernel cannot
    // hold the scene in a workgroup's LDS: the class tables and per-tile state of the wavefront kernel, the object records of the simple one.
    const size_t lds = (ctx->cfg.flags & RT_FLAG_SIMPLE) ? (size_t) sd->n_objects * sizeof(DevObject)
                                                         : rt_wavefront_lds_bytes_strict(fa.stage_bytes, sd->n_lights, (int) fa.has_mirror, fa.cull ? fa.n_us : 0u, 0, fa.n_cub);
    // Which kernels are the halo, G and refine passes of an adaptive frame?  The streamed ones where the caller allows them
    // (RT_FLAG_STREAM_ADAPTIVE) and the staged ones cannot take the context: one decision, before the refusals it lifts.
    const size_t ray_lds = (size_t) sd->n_objects * (sizeof(DevObject) + sizeof(UsEntry));
    ctx->stream_adaptive = ctx->adaptive && (ctx->cfg.flags & RT_FLAG_STREAM_ADAPTIVE) &&
                           ((ctx->cfg.flags & RT_FLAG_STREAM) || (!(ctx->cfg.flags & RT_FLAG_SIMPLE) && lds > 160u * 1024u) || ray_lds > 160u * 1024u ||
                            (ctx->geometry && rt_gbuffer_lds_bytes_strict(&fa) > 160u * 1024u));
    if (ctx->stream_adaptive && (ctx->cfg.flags & RT_FLAG_COUNT))
        return fail(RT_ERR_SCENE, "rt_create: the adaptive passes of this context are the streamed ones (RT_FLAG_STREAM_ADAPTIVE), and the streamed passes book no counters "
                                  "(RT_FLAG_COUNT)");
    if (ctx->adaptive && !ctx->stream_adaptive && !(ctx->cfg.flags & RT_FLAG_SIMPLE) && lds > 160u * 1024u) // (without RT_FLAG_STREAM_ADAPTIVE: refused as ever)
        return fail(RT_ERR_SCENE, "rt_create: scene needs %zu bytes of LDS per workgroup (limit 160 KiB)", lds);
    ctx->streamed = (ctx->cfg.flags & RT_FLAG_STREAM) || lds > 160u * 1024u;
    if (ctx->streamed) ctx->lean_ok = false;
    // ... and which kernels are the queries?  One decision per context: rt_set_scene cannot change the layout.
    ctx->stream_queries = (ctx->cfg.flags & RT_FLAG_STREAM_QUERIES) && (ctx->streamed || rt_gbuffer_lds_bytes_strict(&fa) > 160u * 1024u);
    if (ctx->adaptive && !ctx->stream_adaptive && ray_lds > 160u * 1024u)
        return fail(RT_ERR_SCENE, "rt_create: adaptive supersampling stages %zu bytes of LDS per workgroup (limit 160 KiB)", ray_lds);
    if (ctx->streamed && (ctx->cfg.flags & RT_FLAG_COUNT)) // (RT_FLAG_STREAM itself was refused in create_checks: this is streaming forced by the scene's size, RT_FLAG_SIMPLE contexts included)
        return fail(RT_ERR_SCENE, "rt_create: scene needs %zu bytes of LDS per workgroup (limit 160 KiB), so it takes the streamed kernel, and the streamed kernel books no counters "
                                  "(RT_FLAG_COUNT)", lds);
    if (ctx->geometry && !ctx->stream_adaptive && rt_gbuffer_lds_bytes_strict(&fa) > 160u * 1024u)
        return fail(RT_ERR_SCENE, "rt_create: RT_FLAG_SSAA_GEOMETRY stages %zu bytes of LDS per workgroup (limit 160 KiB)", rt_gbuffer_lds_bytes_strict(&fa));
    // Does rt_render cull whole chunks of the unit-sphere table (rt_stream_cull.hip)?  One decision, as above.  True: the table takes the
    // context's spatial order and every chunk gets its bound (rt_scene_image.hpp); false: nothing of the context differs from one without the flag.
    // ... and do the culling families keep work words?  Asked once, here: a decision below and the allocation in create_device_state both go by it.
    const char *stats_env = std::getenv("MI355RT_STREAM_CULL_STATS");
    ctx->words_wanted = stats_env && !std::strcmp(stats_env, "1");
    bool *cull = ctx->cull;
    cull[CULL_FRAME] = (ctx->cfg.flags & RT_FLAG_STREAM_CULL) && ctx->streamed && fa.cull;
    if (cull[CULL_FRAME]) {
        im.bounds = rtp::stream_cull_image(im, fa);
        ctx->n_chunks = (uint32_t) im.bounds.size();
    }
    // ... and can rt_reorder_scene put that table back into this order after rt_set_scene has moved the spheres (rt_reorder_scene.hip)?  The flag and the
    // decision above.  False: call for call the context without the flag -- no work space, and rt_reorder_scene enqueues nothing.
    ctx->reorder = (ctx->cfg.flags & RT_FLAG_STREAM_CULL_REORDER) && cull[CULL_FRAME];
    // ... and do the halo and refine passes cull them too (rt_stream_cull_adaptive.hip)?  Both decisions above, and a second chunk: with one,
    // the chunk level can remove nothing and is paid per query.
    cull[CULL_ADAPTIVE] = cull[CULL_FRAME] && ctx->stream_adaptive && ctx->n_chunks >= 2u;
    // ... and does rt_render cull its bounce rays per ray (rt_stream_cull_bounce.hip)?  The decision above, a scene and a context in which a ray
    // can bounce at all, and a second chunk.  False: launch for launch the context without the flag.  rt_set_scene keeps has_mirror and the chunk
    // layout, so this holds for the context's life.
    cull[CULL_BOUNCE] = (ctx->cfg.flags & RT_FLAG_STREAM_CULL_BOUNCE) && cull[CULL_FRAME] && fa.has_mirror && fa.max_refl >= 1u && ctx->n_chunks >= 2u;
    // ... and do the ray queries cull the chunks per caller-supplied ray (rt_stream_cull_rays.hip)?  The culling decision, streamed queries and a second
    // chunk.  False: launch for launch the context without the flag.  rt_set_scene rebuilds the bounds and keeps the layout, so this holds too.
    cull[CULL_RAYS] = (ctx->cfg.flags & RT_FLAG_STREAM_CULL_RAYS) && cull[CULL_FRAME] && ctx->stream_queries && ctx->n_chunks >= 2u;
    // ... and do the pixel queries cull the chunks by the block's cone (rt_stream_cull_pixels.hip)?  The same three conditions under a flag of its own.
    // False: launch for launch the context without the flag.  (cull[CULL_FRAME] implies fa.cull: the cone exists.)
    cull[CULL_PIXELS] = (ctx->cfg.flags & RT_FLAG_STREAM_CULL_PIXELS) && cull[CULL_FRAME] && ctx->stream_queries && ctx->n_chunks >= 2u;
    // ... and does rt_render ask a second level of bounds first, one per 64 chunk bounds (rt_stream_cull_groups.hip)?  The flag, the culling decision and a
    // second group: with one, the group level can remove nothing and is paid per query.  False: launch for launch the context without the flag.  rt_set_scene
    // and rt_reorder_scene keep the chunk layout, so this holds for the context's life.
    ctx->n_groups = (ctx->n_chunks + 63u) / 64u;
    // One instantiation is not built (rt_stream_cull_groups.hip): the kernel that counts and culls bounce rays for general quadrics plus degree 3.  A context
    // that would need it -- such a scene, a true bounce decision and the work words asked for -- is the context without the flag.
    const bool not_built = fa.n_gq && fa.n_cub && cull[CULL_BOUNCE] && ctx->words_wanted;
    ctx->groups = (ctx->cfg.flags & RT_FLAG_STREAM_CULL_GROUPS) && cull[CULL_FRAME] && ctx->n_groups >= 2u && !not_built;
    if (ctx->groups) im.groups = rtp::stream_group_image(im.bounds);
    else ctx->n_groups = 0u;
    // So the launchers the query entry points call, for the context's life: the culled path where the family culls, else the streamed or the staged one.
    const TablePath plain = ctx->stream_queries ? PATH_STREAMED : PATH_STAGED;
    ctx->pixel_q = &ctx->kern->query[cull[CULL_PIXELS] ? PATH_CULLED : plain];
    ctx->ray_q = &ctx->kern->query[cull[CULL_RAYS] ? PATH_CULLED : plain];
    return RT_OK;
}

// 4. what every context holds on the device: scene, framebuffer, counters, events, the camera-plane tables
static int create_device_state(rt_ctx *ctx, const rtp::SceneImage &im)
{
    const FrameArgs &fa = ctx->fa;
    const size_t nl = im.lights.size();
    if (int rc = device_table(ctx->d_obj, im.blob.data(), im.blob.size(), "scene")) return rc;
    RT_TRY("hipMalloc(lights)", ctx->d_light.alloc((sizeof(DevLight) + sizeof(LightK)) * (nl ? nl : 1)));
    if (nl) {
        RT_TRY("hipMemcpy(lights)", hipMemcpy(ctx->d_light, im.lights.data(), sizeof(DevLight) * nl, hipMemcpyHostToDevice));
        RT_TRY("hipMemcpy(light table)", hipMemcpy(ctx->d_light + nl, im.lightk.data(), sizeof(LightK) * nl, hipMemcpyHostToDevice));
    }
    RT_TRY("hipMalloc(framebuffer)", ctx->d_fb.alloc((size_t) (ctx->local_rows ? ctx->local_rows : 1) * ctx->width * ctx->pixel_bytes));
    if (int rc = device_table(ctx->d_counters, nullptr, sizeof(unsigned long long) * 64, "counters")) return rc;
    if (int rc = device_table(ctx->d_ss_status, nullptr, sizeof(SetSceneStatus), "scene-update status")) return rc;
    if (ctx->cull[CULL_FRAME]) {
        if (int rc = device_table(ctx->d_bounds, im.bounds.data(), sizeof(UsEntry) * im.bounds.size(), "chunk bounds")) return rc;
        const char *e = ctx->words_wanted ? "1" : nullptr; // (MI355RT_STREAM_CULL_STATS as create_scene read it: one reading for the decisions and the words)
        if (e && !std::strcmp(e, "1"))
            if (int rc = device_table(ctx->d_cull_words, nullptr, sizeof(unsigned long long) * 8 * N_CULL_FAMILIES, "stream-cull work words")) return rc;
        // a family that culls takes the bounds, and its own 8 words where there are any (the adaptive kernel that counts for a scene with both general
        // quadrics and degree-3 objects is not built: no words there)
        for (int f = 0; f < N_CULL_FAMILIES; f++) {
            const bool words = ctx->d_cull_words && !(f == CULL_ADAPTIVE && fa.n_gq && fa.n_cub);
            if (ctx->cull[f]) ctx->chunks[f] = ChunkTables{ctx->d_bounds.p, ctx->n_chunks, words ? ctx->d_cull_words + 8 * f : nullptr};
        }
    }
    if (ctx->groups) {
        if (int rc = device_table(ctx->d_groups, im.groups.data(), sizeof(UsEntry) * im.groups.size(), "group bounds")) return rc;
        if (ctx->d_cull_words)
            if (int rc = device_table(ctx->d_group_words, nullptr, sizeof(unsigned long long) * 8, "stream-cull group work words")) return rc;
        ctx->group_tables = GroupTables{ctx->d_groups.p, ctx->n_groups, ctx->d_group_words.p};
    }
    if (ctx->reorder) {
        RT_TRY("hipMalloc(reorder work space)", ctx->d_reorder_work.alloc(rt_reorder_scene_work_size(fa.n_us)));
        ctx->reorder_max_grid = ctx->wg_slots / 6u * 4u;
        if (const char *e = std::getenv("MI355RT_REORDER_MAX_GRID")) {
            char *end = nullptr;
            const unsigned long v = std::strtoul(e, &end, 10);
            if (!*e || *end || v == 0ul || v > 65535ul) return fail(RT_ERR_INVALID, "rt_create: MI355RT_REORDER_MAX_GRID=%s: expected a number of workgroups, 1 .. 65535", e);
            ctx->reorder_max_grid = (uint32_t) v;
        }
    }
    RT_TRY("hipEventCreate", ctx->ev0.create());
    RT_TRY("hipEventCreate", ctx->ev1.create());
    RT_TRY("hipEventCreate", ctx->ev_done.create(hipEventDisableTiming));
    if (ctx->ssaa > 1u && !ctx->adaptive) RT_TRY("hipMalloc(supersampled frame)", ctx->d_ss.alloc((size_t) (fa.local_rows ? fa.local_rows : 1) * fa.width * 16u));
    std::vector<double> cx, cy;
    rtf::camera_tables(fa.width, fa.height, fa.aspect, fa.tan_half_fov, cx, cy);
    if (int rc = device_table(ctx->d_camx, cx.data(), sizeof(double) * cx.size(), "camx")) return rc;
    return device_table(ctx->d_camy, cy.data(), sizeof(double) * cy.size(), "camy");
}

// workgroups of ray_list_stream_kernel a CU holds: the occupancy build/spills.txt reports for its instantiations (waves per SIMD; a workgroup is one wave per SIMD)
constexpr uint32_t SA_WG_PER_CU = 2;

// 5. RT_FLAG_SSAA_ADAPTIVE / RT_FLAG_SSAA_GEOMETRY: the refine list, the halo rows, the sample grid's tables, the primary-hit planes
static int create_adaptive(rt_ctx *ctx)
{
    const rt_config &cfg = ctx->cfg;
    const FrameArgs &fa = ctx->fa;
    const uint32_t k = ctx->ssaa, width = ctx->width, height = ctx->height;
    const size_t px = (size_t) ctx->local_rows * width;
    const uint32_t bands = (ctx->local_rows + cfg.band_rows - 1u) / cfg.band_rows;
    ctx->halo_slots = cfg.world > 1u ? 2u * bands : 0u;
    for (uint32_t h = 0; h < ctx->halo_slots; h++) {
        const int64_t gy = rtf::halo_global_row(h, cfg.band_rows, cfg.world, cfg.rank, ctx->local_rows);
        if (gy >= 0 && gy < (int64_t) height) ctx->halo_rays += width;
    }
    // the ray-list kernel keeps one workgroup per CU resident (it needs all 512 registers of a lane); twice that many keeps every CU
    // busy while the last workgroups drain
    const uint64_t ppw = 64u / (k * k), want = (px + ppw * 4u - 1u) / (ppw * 4u), hwant = ((uint64_t) ctx->halo_slots * width + 255u) / 256u;
    // (the streamed twin keeps SA_WG_PER_CU workgroups per CU resident -- its registers, build/spills.txt -- and its waves share nothing, so the
    // grid is exactly the resident set: wg_slots = 6 per CU)
    const uint32_t slots = ctx->stream_adaptive ? ctx->wg_slots * SA_WG_PER_CU / 6u : ctx->wg_slots / 3u;
    const uint32_t cap = slots ? slots : 1u;
    ctx->ray_grid = (uint32_t) std::min<uint64_t>(want, cap);
    ctx->halo_grid = (uint32_t) std::min<uint64_t>(hwant, cap);
    RT_TRY("hipMalloc(refine list)", ctx->d_list.alloc(sizeof(uint32_t) * (px + 1u)));
    if (cfg.format == RT_FMT_RGBA8) RT_TRY("hipMalloc(plain frame)", ctx->d_p.alloc((px ? px : 1u) * 16u));
    if (ctx->halo_slots) RT_TRY("hipMalloc(halo rows)", ctx->d_halo.alloc((size_t) ctx->halo_slots * width * 16u));
    RT_TRY("hipMemset(refine count)", hipMemset(ctx->d_list + px, 0, sizeof(uint32_t)));
    std::vector<double> cx, cy; // the tables of the k-times finer frame, exactly as a RT_FLAG_SSAAk context forms its own
    rtf::camera_tables(k * width, k * height, fa.aspect, fa.tan_half_fov, cx, cy);
    if (int rc = device_table(ctx->d_camxk, cx.data(), sizeof(double) * cx.size(), "camx")) return rc;
    if (int rc = device_table(ctx->d_camyk, cy.data(), sizeof(double) * cy.size(), "camy")) return rc;
    if (!ctx->geometry) return RT_OK;
    // the halo rows' pixels by global coordinates, slot-major like d_halo; a slot outside the image is never read by the
    // classifier: it traces the nearest image row, so that every query is a valid one
    const size_t hpx = (size_t) ctx->halo_slots * width;
    std::vector<uint32_t> xy(2u * hpx);
    for (uint32_t h = 0; h < ctx->halo_slots; h++) {
        const int64_t gy = rtf::halo_global_row(h, cfg.band_rows, cfg.world, cfg.rank, ctx->local_rows);
        const uint32_t row = (uint32_t) std::min<int64_t>(std::max<int64_t>(gy, 0), (int64_t) height - 1);
        for (uint32_t x = 0; x < width; x++) {
            xy[2u * ((size_t) h * width + x)] = x;
            xy[2u * ((size_t) h * width + x) + 1u] = row;
        }
    }
    RT_TRY("hipMalloc(object plane)", ctx->d_geo_obj.alloc((px ? px : 1u) * sizeof(int32_t)));
    RT_TRY("hipMalloc(normal plane)", ctx->d_geo_nrm.alloc((px ? px : 1u) * 16u));
    if (!hpx) return RT_OK;
    RT_TRY("hipMalloc(halo records)", ctx->d_geo_halo.alloc(sizeof(rt_hit) * hpx));
    return device_table(ctx->d_geo_xy, xy.data(), sizeof(uint32_t) * 2u * hpx, "halo coordinates");
}

// 6. the frame-to-frame state of the wavefront kernel: launch-order generations, the host-mapped words, tile words (and stamp rows)
static int create_order_state(rt_ctx *ctx)
{
    FrameArgs &fa = ctx->fa;
    const uint32_t flags = ctx->cfg.flags;
    const bool stateless = (flags & RT_FLAG_SIMPLE) || ctx->streamed; // one kernel per frame that reads nothing an earlier frame left
    if (!stateless && !(flags & RT_FLAG_STATIC_ORDER) && fa.n_tiles > 0 && fa.n_tiles <= RT_ORD_MAX_TILES) {
        // launch-order feedback: three generations, all empty (first frame = index order)
        fa.ord_stride = (RT_ORD_HDR + 17u * fa.n_tiles + 15u) & ~15u;
        // ... and behind them one word per tile, the last frame in which one of a split tile's two workgroups entered the tile (FrameArgs::ord_frame)
        if (int rc = device_table(ctx->d_order, nullptr, sizeof(uint32_t) * (3u * (size_t) fa.ord_stride + fa.n_tiles), "order")) return rc;
        fa.order_state = ctx->d_order;
        // the kernel reports the number of listed tiles through one host-mapped word; without it (allocation
        // refused) every launch simply carries n_tiles list slots
        if (hipHostMalloc((void **) &ctx->h_listed.p, 64, hipHostMallocMapped | hipHostMallocPortable) == hipSuccess) {
            ctx->h_listed[0] = 0;
            ctx->h_listed[1] = 0;
            ctx->h_listed[2] = 0xFFFFFFFFu; // (nothing known yet: the wave-per-block instantiation starts)
            if (hipHostGetDevicePointer((void **) &fa.ord_host, ctx->h_listed, 0) != hipSuccess) {
                ctx->h_listed.reset();
                fa.ord_host = nullptr;
            }
        } else {
            ctx->h_listed.p = nullptr;
            (void) hipGetLastError();
        }
    }
    if (!stateless && fa.all_cullable && fa.n_tiles > 0) {
        // one word per tile for the scan workgroups (rt_wavefront.hip, scan_tiles); all zero = "no frame has classified it"
        if (int rc = device_table(ctx->d_tiles, nullptr, sizeof(uint32_t) * fa.n_tiles, "tile state")) return rc;
        fa.tile_state = ctx->d_tiles;
    }
    ctx->zero_counters = std::getenv("MI355RT_DEBUG_COUNTERS") != nullptr;
    if (ctx->zero_counters) { // room for the stamp rows of a diagnostic (STAMPS=1) build: one per wave
        ctx->n_stamp_rows = (size_t) fa.n_tiles * 9 + 96; // one row per wave of the (up to) 2 * n_tiles + n_tiles / 16 + n_tiles / 64 + 2 workgroups of a launch
        if (ctx->d_stamps.alloc(ctx->n_stamp_rows * 16 * sizeof(uint64_t) + 8) != hipSuccess) ctx->d_stamps.p = nullptr;
        else (void) hipMemset(ctx->d_stamps, 0, ctx->n_stamp_rows * 16 * sizeof(uint64_t));
    }
    return RT_OK;
}

extern "C" int rt_create(rt_ctx **out, const rt_scene_desc *sd, const rt_config *cfg_in)
{
    if (!out || !sd) return fail(RT_ERR_INVALID, "rt_create: null argument");
    *out = nullptr;
    return guarded(RT_ERR_INVALID, [&]() -> int { // host-side packing allocates; nothing may propagate through the C ABI
        // owned here until the very end: whatever throws or fails on the way, the context goes, and with it every device buffer it
        // already holds (its device is current from the first allocation on)
        std::unique_ptr<rt_ctx> ctx(new rt_ctx());
        if (int rc = create_checks(ctx.get(), sd, cfg_in)) return rc;
        int ndev = 0, device = ctx->cfg.device;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0)
            return fail(RT_ERR_NO_DEVICE, "rt_create: no HIP device available (%s); this library has no CPU fallback",
                        e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        if (device < 0) RT_HIP(hipGetDevice(&device));
        if (device >= ndev) return fail(RT_ERR_INVALID, "rt_create: device %d out of range (%d devices)", device, ndev);
        RT_HIP(hipSetDevice(device));
        rtp::SceneImage im;
        create_frame(ctx.get(), sd, device);
        if (int rc = create_scene(ctx.get(), sd, im)) return rc;
        if (int rc = create_device_state(ctx.get(), im)) return rc;
        if (ctx->adaptive)
            if (int rc = create_adaptive(ctx.get())) return rc;
        if (int rc = create_order_state(ctx.get())) return rc;
        *out = ctx.release();
        return RT_OK;
    });
}

// background colour as the RGBA8 kernels store it (iround(c * 255), alpha 255), little-endian r | g << 8 | b << 16 | a << 24
static uint32_t bg_rgba8(const FrameArgs &fa)
{
    const uint32_t r = (uint32_t) (unsigned char) (int) (fa.bg[0] * 255.0f + 0.5f), g = (uint32_t) (unsigned char) (int) (fa.bg[1] * 255.0f + 0.5f),
                   b = (uint32_t) (unsigned char) (int) (fa.bg[2] * 255.0f + 0.5f);
    return r | (g << 8) | (b << 16) | (255u << 24);
}

// the background pixel of the context's format as four words (what the sparse kernels compare with and paint): RGBA8 in word 0,
// RGBA32F the bits of (bg_color, 1.0f) -- what the render kernels store for a pixel without hits
struct BgPixel {
    uint32_t w[4];
};
static BgPixel bg_pixel(const rt_ctx *ctx)
{
    BgPixel p{};
    if (ctx->cfg.format == RT_FMT_RGBA8) {
        p.w[0] = bg_rgba8(ctx->fa);
    } else {
        const float f[4] = {ctx->fa.bg[0], ctx->fa.bg[1], ctx->fa.bg[2], 1.0f};
        std::memcpy(p.w, f, sizeof(f));
    }
    return p;
}

// ---- what every entry point on a context shares ----------------------------------------------------------------
static int use_device(const rt_ctx *ctx) // make the context's device the calling thread's current one
{
    int cur = -1;
    RT_HIP(hipGetDevice(&cur));
    if (cur != ctx->device) RT_HIP(hipSetDevice(ctx->device));
    return RT_OK;
}

// wait for everything the device has been given, then copy back (the getters)
static int read_synced(const rt_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (int rc = use_device(ctx)) return rc;
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

// A context's frames depend on each other on the device (launch-order generations: read k, append k + 1, clear k + 2; tile words
// tagged per frame), and a scene update belongs between two of them, so its calls must run in the order they were issued.  On one
// stream they do; when the caller switches streams, the new stream first waits for the previous call (order_begin), and every call
// leaves the event the next one may have to wait for (order_end).
static int order_begin(const char *who, rt_ctx *ctx, hipStream_t stream, bool *capturing)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream) RT_HIP(hipStreamIsCapturing(stream, &cap));
    *capturing = cap != hipStreamCaptureStatusNone;
    if (ctx->rendered && stream != ctx->last_stream) {
        if (ctx->captured || *capturing)
            return fail(RT_ERR_INVALID, "%s: a context whose calls were captured into a graph on one stream must stay on that stream (frames and scene updates of a "
                                        "context are ordered on the device, and a capture cannot be ordered against another stream through an event)", who);
        RT_HIP(hipStreamWaitEvent(stream, ctx->ev_done, 0));
    }
    return RT_OK;
}

static int order_end(rt_ctx *ctx, hipStream_t stream, bool capturing)
{
    if (!capturing) RT_HIP(hipEventRecord(ctx->ev_done, stream));
    ctx->captured = capturing;
    ctx->last_stream = stream;
    ctx->rendered = true;
    return RT_OK;
}

// `ms` of a timed entry point: the device time between the two calls (timer_end waits for it); nothing when ms is null
static int timer_begin(rt_ctx *ctx, hipStream_t stream, const float *ms)
{
    if (ms) RT_HIP(hipEventRecord(ctx->ev0, stream));
    return RT_OK;
}

static int timer_end(rt_ctx *ctx, hipStream_t stream, float *ms)
{
    if (!ms) return RT_OK;
    RT_HIP(hipEventRecord(ctx->ev1, stream));
    RT_HIP(hipEventSynchronize(ctx->ev1));
    RT_HIP(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return RT_OK;
}

// ---- rt_render ----------------------------------------------------------------------------------------------
// Which instantiation renders a scene of unit spheres?  The wave-per-block one ("lean") executes a quarter fewer instructions per
// frame and wins wherever the GPU is full (4K 120 -> 91 us, 8K 425 -> 306, the 1080p start pose 44 -> 38).  The general one splits
// costly tiles over two workgroups and every tile's lights over its four waves, which is what counts while few tiles have hits and
// the frame ends with its slowest wave (orbit poses 5 / 6 at 1080p: 40 us against 54).  The previous frames' count of tiles with
// hits decides, with a hysteresis: lean from 0.66 of the workgroup slots up, back below 0.62 (the orbit of tools/flythrough_bench.py: the
// general one wins every pose below 950 tiles for 1536 slots and loses every pose above 975; a wider band kept poses 3 and 4 on the wrong side).
static void choose_schedule(rt_ctx *ctx, FrameArgs &fa)
{
    if (ctx->lean_ok && ctx->h_listed && ctx->lean_force == 0) {
        const uint32_t tiles = ((volatile uint32_t *) ctx->h_listed.p)[2]; // tiles with hits a few frames ago (listed, or the census' estimate while the lists are off)
        if (ctx->lean_now ? (uint64_t) tiles * 100u < (uint64_t) ctx->wg_slots * 62u : (uint64_t) tiles * 100u >= (uint64_t) ctx->wg_slots * 66u) ctx->lean_now = !ctx->lean_now;
    } else {
        ctx->lean_now = ctx->lean_force >= 0;
    }
    static const bool debug_order = std::getenv("MI355RT_DEBUG_ORDER") != nullptr; // (diagnostics: what the previous frames' kernels reported back)
    if (debug_order && ctx->h_listed)
        std::fprintf(stderr, "mi355rt: frame %llu: tiles with hits %u, list slots wanted %u, census %u, schedule %s\n", (unsigned long long) ctx->frame, ((volatile uint32_t *) ctx->h_listed.p)[2],
                     ((volatile uint32_t *) ctx->h_listed.p)[0], ((volatile uint32_t *) ctx->h_listed.p)[1], ctx->lean_now ? "lean" : "general");
    fa.lean = (ctx->lean_ok && ctx->lean_now && !fa.sparse) ? 1u : 0u;
}

// rotate the launch-order generations: read k, write k+1, clear k+2 (contexts with FrameArgs::order_state)
static int rotate_launch_order(rt_ctx *ctx, FrameArgs &fa, hipStream_t stream)
{
    fa.ord_read = (uint32_t) (ctx->frame % 3u);
    fa.ord_write = (uint32_t) ((ctx->frame + 1u) % 3u);
    fa.ord_zero = (uint32_t) ((ctx->frame + 2u) % 3u);
    // list slots of this launch: what an earlier frame reported (the host runs ahead of the device, so the words
    // are a few frames old) plus a quarter and 64; too few only means that the surplus tiles start in index order.
    // The ordering is switched off while the census says that >= 25 % of the tiles have hits (back on below 20 %).
    uint32_t cap = fa.n_tiles;
    if (ctx->h_listed) {
        const uint32_t seen = ((volatile uint32_t *) ctx->h_listed.p)[0], census = ((volatile uint32_t *) ctx->h_listed.p)[1];
        const uint64_t want = (uint64_t) seen + seen / 4u + 64u;
        if (want < cap) cap = (uint32_t) want;
        const uint64_t with_hits = (uint64_t) census * 16u;
        // ... and while so many tiles have hits that the launch is many rounds of workgroups deep anyway: there the order buys nothing any
        // more and the lists only cost their upkeep -- the decode in front of every list slot.  Measured with the lean schedule (index
        // order against lists): 2 rounds (4K orbit pose 5) 81 -> 69 us with the lists, 3.7 rounds (4K pose 19) 117 -> 109, 4.3 rounds (4K pose
        // 16) 119 / 120, 7.5 - 8 rounds (8K poses 5 / 6) 206 -> 243 and 197 -> 233, 12.7 rounds (8K start pose) 288 / 293.  Off from 16 / 3
        // rounds, back on below 4.
        const uint64_t slots = ctx->wg_slots ? ctx->wg_slots : 1536u;
        const bool too_many = ctx->ord_on ? with_hits * 3u >= slots * 16u : with_hits >= slots * 4u;
        const bool too_dense = ctx->ord_on ? with_hits * 4u >= fa.n_tiles : with_hits * 5u >= fa.n_tiles;
        ctx->ord_on = !(too_many || too_dense);
    }
    fa.ord_cap = cap;
    fa.ord_on = ctx->ord_on ? 1u : 0u;
    fa.ord_split = (fa.sparse || fa.lean) ? 0u : ctx->ord_split; // (a sparse message has one slot per tile; the lean instantiation's waves are independent:
                                                                 // a second workgroup per tile would shorten nothing)
    // this frame's number for the per-tile "entered by" words of split tiles: 1 .. 0xFFFFFFF0, never 0 (the words start out 0).  The
    // election is an atomicMax, so when the number starts over (every 2^32 - 16 frames) the words are cleared first -- the same
    // guard the tile-word tag has in render_impl.
    fa.ord_frame = (uint32_t) (ctx->frame % 0xFFFFFFF0ull) + 1u;
    if (fa.ord_frame == 1u && ctx->frame != 0u)
        RT_HIP(hipMemsetAsync(fa.order_state + 3u * (size_t) fa.ord_stride, 0, sizeof(uint32_t) * fa.n_tiles, stream));
    ctx->frame++;
    return RT_OK;
}

// One pass of an adaptive frame over a ray list (the halo rows: k = 1, n_items slots; the refine pass: k = the context's, the device-side count): the
// staged kernel (rt_adaptive.hip) or, on a context whose adaptive passes are streamed -- rt_ctx::stream_adaptive, rt_ctx::cull[CULL_ADAPTIVE], decided once
// in rt_create --, that pass's streamed or culled twin.  The streamed passes book no counters.  One graph node.
static hipError_t ray_list_launch(rt_ctx *ctx, const double *camx, const double *camy, const uint32_t *list, const uint32_t *count_ptr, uint32_t n_items, uint32_t k, uint32_t grid,
                                  void *out, int rgba8, int count, hipStream_t stream)
{
    const Kernels *kern = ctx->kern;
    if (ctx->cull[CULL_ADAPTIVE])
        return kern->stream_cull_ray_list(&ctx->fa, ctx->d_obj, ctx->d_light, camx, camy, list, count_ptr, n_items, k, grid, out, rgba8, &ctx->chunks[CULL_ADAPTIVE], stream);
    if (ctx->stream_adaptive) return kern->stream_ray_list(&ctx->fa, ctx->d_obj, ctx->d_light, camx, camy, list, count_ptr, n_items, k, grid, out, rgba8, stream);
    return kern->ray_list(&ctx->fa, ctx->d_obj, ctx->d_light, camx, camy, list, count_ptr, n_items, k, grid, out, rgba8, count, ctx->d_counters, stream);
}

static int render_impl(rt_ctx *ctx, const double cam[16], void *dev_fb, void *stream_, float *ms, bool sparse, uint32_t sparse_cap)
{
    hipStream_t stream = (hipStream_t) stream_;
    FrameArgs &fa = ctx->fa;
    const bool ss = ctx->ssaa > 1u && !ctx->adaptive; // supersampled: render the internal frame densely, resolve, and (sparse) pack the resolved rows
    const bool kernel_sparse = sparse && ctx->ssaa == 1u; // (adaptive frames are packed like supersampled ones)
    fa.sparse = kernel_sparse ? 1u : 0u;
    fa.sparse_cap = kernel_sparse ? sparse_cap : 0u;
    choose_schedule(ctx, fa);
    rtf::frame_camera(fa, cam, ctx->cub_coefs);
    if (int rc = use_device(ctx)) return rc;
    bool capturing = false;
    if (int rc = order_begin("rt_render", ctx, stream, &capturing)) return rc;
    // out: where the frame ends up (a message for sparse calls); fb: what the render kernels write
    void *out = dev_fb ? dev_fb : ctx->d_fb.p;
    void *fb = ss ? ctx->d_ss.p : out;
    // dest: where the output rows of a supersampled or adaptive frame go before a sparse pack; the plain frame P is rendered in place for RGBA32F
    void *dest = sparse ? ctx->d_fb.p : out;
    if (ctx->adaptive) fb = ctx->cfg.format == RT_FMT_RGBA8 ? ctx->d_p.p : dest;
    if (kernel_sparse) RT_HIP(hipMemsetAsync(fb, 0, 16, stream)); // message header: count, overflow
    const int count = (ctx->cfg.flags & RT_FLAG_COUNT) ? 1 : 0;
    if (count || ctx->zero_counters) {
        RT_HIP(hipMemsetAsync(ctx->d_counters, 0, sizeof(unsigned long long) * 28, stream)); // (word 31 holds the stamp rows' address)
        RT_HIP(hipMemsetAsync(ctx->d_counters + 32, 0, sizeof(unsigned long long) * 32, stream));
    }
    if (ctx->d_stamps) {
        RT_HIP(hipMemsetAsync(ctx->d_stamps, 0, ctx->n_stamp_rows * 16 * sizeof(uint64_t), stream)); // rows of this frame only
        const unsigned long long ptr = (unsigned long long) (uintptr_t) ctx->d_stamps.p;
        RT_HIP(hipMemcpyAsync(ctx->d_counters + 31, &ptr, sizeof(ptr), hipMemcpyHostToDevice, stream));
        RT_HIP(hipStreamSynchronize(stream));
    }
    fa.n_scan = 0;
    if (fa.tile_state && fa.tile_planes_ok && !(ctx->cfg.flags & RT_FLAG_NOSCAN)) {
        if (ctx->tag >= 0x1FFFFFF0u) { // the tag is stored shifted by three bits: start over with clean words (once in 2^29 frames)
            RT_HIP(hipMemsetAsync(fa.tile_state, 0, sizeof(uint32_t) * fa.n_tiles, stream));
            ctx->tag = 0;
        }
        fa.frame_tag = ++ctx->tag;
        fa.n_scan = (fa.n_tiles + RT_SCAN_TILES - 1) / RT_SCAN_TILES;
    }
    if (fa.order_state)
        if (int rc = rotate_launch_order(ctx, fa, stream)) return rc;
    if (int rc = timer_begin(ctx, stream, ms)) return rc;
    const ChunkTables *frame_chunks = &ctx->chunks[CULL_FRAME]; // (the bounce kernel books the frame's words as well as its own)
    const hipError_t e = ctx->groups ? ctx->group_kern->frame(&fa, ctx->d_obj, ctx->d_light, ctx->d_camx, ctx->d_camy, fb, frame_chunks, &ctx->group_tables, ctx->chunks[CULL_BOUNCE].stats, ctx->cull[CULL_BOUNCE], stream)
                         : ctx->cull[CULL_BOUNCE] ? ctx->kern->stream_cull_bounce(&fa, ctx->d_obj, ctx->d_light, ctx->d_camx, ctx->d_camy, fb, frame_chunks, ctx->chunks[CULL_BOUNCE].stats, stream)
                         : ctx->cull[CULL_FRAME] ? ctx->kern->stream_cull(&fa, ctx->d_obj, ctx->d_light, ctx->d_camx, ctx->d_camy, fb, frame_chunks, stream)
                         : ctx->streamed ? ctx->kern->stream(&fa, ctx->d_obj, ctx->d_light, ctx->d_camx, ctx->d_camy, fb, stream)
                         : (ctx->cfg.flags & RT_FLAG_SIMPLE) ? ctx->kern->trace(&fa, ctx->d_obj, ctx->d_light, fb, ctx->d_counters, fa.rgba8 != 0u, count, stream)
                                                           : ctx->kern->wavefront(&fa, ctx->d_obj, ctx->d_light, fb, ctx->d_counters, count, ctx->d_camx, ctx->d_camy, stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(e));
    const int out8 = ctx->cfg.format == RT_FMT_RGBA8;
    if (ctx->adaptive) {
        // halo rows -> clear the list -> classify (unrefined pixels written out) -> the k^2 sample rays of the listed pixels; the next
        // frame's plain pass overwrites what these read, and the ordering event below is recorded behind the last of them
        const size_t px = (size_t) ctx->local_rows * ctx->width;
        if (ctx->halo_slots)
            RT_HIP(ray_list_launch(ctx, ctx->d_camx, ctx->d_camy, nullptr, nullptr, ctx->halo_slots * ctx->width, 1u, ctx->halo_grid, ctx->d_halo, 0, count, stream));
        RT_HIP(hipMemsetAsync(ctx->d_list + px, 0, sizeof(uint32_t), stream));
        if (ctx->geometry) {
            // the primary-hit object (and, for a finite min_cos, normal) of this rank's rows and of the halo rows: gbuffer_kernel itself, which
            // reads no frame state and books no rays; then the classifier with the geometric term
            float *nrm = ctx->min_cos == -INFINITY ? nullptr : ctx->d_geo_nrm.p;
            // (the kernel in its two modes, as rt_render_gbuffer / rt_pick launch it: two nodes with several ranks -- the launchers skip an empty grid --;
            // so the adaptive frame's edges are the ones those two report, in the FAST build too)
            // The path is named here and is never the pixel entry points': streamed where the adaptive passes are, and never culled (its planes equal
            // rt_render_gbuffer's of a culling context by the rule of DESIGN.md section 34, not by identity of kernel).
            const QueryLaunchers &g = ctx->kern->query[ctx->stream_adaptive ? PATH_STREAMED : PATH_STAGED];
            RT_HIP(g.gbuffer(&fa, ctx->d_obj, ctx->d_camx, ctx->d_camy, ctx->d_geo_obj, nullptr, nrm, nullptr, stream));
            RT_HIP(g.pick(&fa, ctx->d_obj, ctx->d_camx, ctx->d_camy, ctx->d_geo_xy, ctx->halo_slots * ctx->width, ctx->d_geo_halo, nullptr, stream));
            RT_HIP(rt_launch_classify_geometry_strict(fb, ctx->d_halo, ctx->d_geo_obj, nrm, ctx->d_geo_halo, ctx->width, ctx->height, ctx->local_rows,
                                                      ctx->cfg.band_rows, ctx->cfg.world, ctx->cfg.rank, ctx->tau, ctx->min_cos, dest, out8, ctx->d_list,
                                                      ctx->d_list + px, stream));
        } else {
            RT_HIP(rt_launch_classify_strict(fb, ctx->d_halo, ctx->width, ctx->height, ctx->local_rows, ctx->cfg.band_rows, ctx->cfg.world, ctx->cfg.rank, ctx->tau,
                                             dest, out8, ctx->d_list, ctx->d_list + px, stream));
        }
        RT_HIP(ray_list_launch(ctx, ctx->d_camxk, ctx->d_camyk, ctx->d_list, ctx->d_list + px, 0u, ctx->ssaa, ctx->ray_grid, dest, out8, count, stream));
    }
    if (ss) // the next frame's render overwrites the internal frame this reads, so the ordering event below is recorded behind it
        RT_HIP(rt_launch_resolve(ctx->d_ss, dest, ctx->width, ctx->local_rows, ctx->ssaa, out8, ctx->resolve_nt, stream));
    if (sparse && !kernel_sparse) { // supersampled and adaptive frames: pack the finished rows into the message
        const BgPixel bg = bg_pixel(ctx);
        RT_HIP(rt_launch_pack_sparse_strict(ctx->d_fb, dev_fb, ctx->width, ctx->local_rows, bg.w, sparse_cap, out8, stream));
    }
    ctx->counted = count != 0;
    if (int rc = order_end(ctx, stream, capturing)) return rc;
    return timer_end(ctx, stream, ms);
}

extern "C" int rt_render(rt_ctx *ctx, const double cam[16], void *dev_fb, void *stream, float *ms)
{
    if (!ctx || !cam) return fail(RT_ERR_INVALID, "rt_render: null argument");
    return render_impl(ctx, cam, dev_fb, stream, ms, false, 0);
}

extern "C" int rt_render_sparse(rt_ctx *ctx, const double cam[16], void *dev_msg, uint32_t capacity_tiles, void *stream, float *ms)
{
    if (!ctx || !cam || !dev_msg) return fail(RT_ERR_INVALID, "rt_render_sparse: null argument");
    if (ctx->cfg.flags & RT_FLAG_SIMPLE) return fail(RT_ERR_INVALID, "rt_render_sparse: not available with RT_FLAG_SIMPLE");
    if (ctx->streamed) return fail(RT_ERR_INVALID, "rt_render_sparse: not available on a streamed context (rt_get_streamed); rt_render and rt_pack_sparse give the same message");
    return render_impl(ctx, cam, dev_msg, stream, ms, true, capacity_tiles);
}

// ---- G-buffer (rt_gbuffer.hip) ---------------------------------------------------------------------------
// The pixel entry points call the launchers rt_create decided on (rt_ctx::pixel_q): the staged, the streamed, or -- RT_FLAG_STREAM_CULL_PIXELS -- the culled
// ones (rt_stream_cull_pixels.hip), which read the family's chunks.  The G pass of an adaptive frame keeps its own two.
// The frame arguments of a G-buffer pass: a COPY of the context's (geometry, scene layout) with this call's camera -- the context's own
// FrameArgs, which carry the render kernels' frame-to-frame state, are neither read for that state nor written.
static int gbuffer_args(const char *who, rt_ctx *ctx, const double cam[16], FrameArgs &fa)
{
    if (ctx->ssaa > 1u || ctx->adaptive)
        return fail(RT_ERR_INVALID, "%s: not available for contexts created with RT_FLAG_SSAA2 / RT_FLAG_SSAA4 / RT_FLAG_SSAA_ADAPTIVE", who);
    fa = ctx->fa;
    fa.order_state = nullptr;
    fa.ord_host = nullptr;
    fa.tile_state = nullptr;
    rtf::frame_origin(fa, cam, ctx->cub_coefs);
    if (!ctx->stream_queries && rt_gbuffer_lds_bytes_strict(&fa) > 160u * 1024u)
        return fail(RT_ERR_SCENE, "%s: scene needs %zu bytes of LDS per workgroup (limit 160 KiB)", who, rt_gbuffer_lds_bytes_strict(&fa));
    return use_device(ctx);
}

extern "C" int rt_render_gbuffer(rt_ctx *ctx, const double cam[16], int32_t *dev_object, double *dev_t, float *dev_normal, void *stream_, float *ms)
{
    if (!ctx || !cam) return fail(RT_ERR_INVALID, "rt_render_gbuffer: null argument");
    if (!dev_object && !dev_t && !dev_normal) return fail(RT_ERR_INVALID, "rt_render_gbuffer: all three planes are null");
    hipStream_t stream = (hipStream_t) stream_;
    FrameArgs fa;
    if (int rc = gbuffer_args("rt_render_gbuffer", ctx, cam, fa)) return rc;
    if (int rc = timer_begin(ctx, stream, ms)) return rc;
    const hipError_t e = ctx->pixel_q->gbuffer(&fa, ctx->d_obj, ctx->d_camx, ctx->d_camy, dev_object, dev_t, dev_normal, &ctx->chunks[CULL_PIXELS], stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "G-buffer kernel launch failed: %s", hipGetErrorString(e));
    return timer_end(ctx, stream, ms);
}

// n pixels by GLOBAL coordinates: all of them are checked before anything is enqueued
static int pixels_inside(const char *who, const rt_ctx *ctx, const uint32_t *xy, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++)
        if (xy[2 * (size_t) i] >= ctx->width || xy[2 * (size_t) i + 1] >= ctx->height)
            return fail(RT_ERR_INVALID, "%s: pixel %u = (%u, %u) lies outside the %u x %u image", who, i, xy[2 * (size_t) i], xy[2 * (size_t) i + 1], ctx->width, ctx->height);
    return RT_OK;
}

extern "C" int rt_pick(rt_ctx *ctx, const double cam[16], const uint32_t *xy, uint32_t n, rt_hit *out_host, void *stream_)
{
    static_assert(sizeof(rt_hit) == 48, "rt_hit layout");
    if (!ctx || !cam || !xy || !out_host) return fail(RT_ERR_INVALID, "rt_pick: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_pick: n is 0");
    if (int rc = pixels_inside("rt_pick", ctx, xy, n)) return rc;
    hipStream_t stream = (hipStream_t) stream_;
    FrameArgs fa;
    if (int rc = gbuffer_args("rt_pick", ctx, cam, fa)) return rc;
    if (int rc = ctx->pick.reserve(n, sizeof(uint32_t) * 2, sizeof(rt_hit))) return rc;
    RT_HIP(hipMemcpyAsync(ctx->pick.in, xy, sizeof(uint32_t) * 2 * (size_t) n, hipMemcpyHostToDevice, stream));
    const hipError_t e = ctx->pixel_q->pick(&fa, ctx->d_obj, ctx->d_camx, ctx->d_camy, (const uint32_t *) ctx->pick.in.p, n, ctx->pick.out, &ctx->chunks[CULL_PIXELS], stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "pick kernel launch failed: %s", hipGetErrorString(e));
    RT_HIP(hipMemcpyAsync(out_host, ctx->pick.out, sizeof(rt_hit) * (size_t) n, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

// ---- object extents (rt_gbuffer.hip) ----------------------------------------------------------------------
// A caller's rectangle of GLOBAL pixels (x0, y0, x1, y1 inclusive; NULL = the whole frame) as r[4], or why it is none
static int rect_args(const char *who, const rt_ctx *ctx, const uint32_t *rect, uint32_t r[4])
{
    if (rect && (rect[0] > rect[2] || rect[1] > rect[3])) // (decided without reading the context)
        return fail(RT_ERR_INVALID, "%s: rect = (%u, %u) .. (%u, %u) is not a rectangle: x0 > x1 or y0 > y1", who, rect[0], rect[1], rect[2], rect[3]);
    if (rect && (rect[2] >= ctx->width || rect[3] >= ctx->height))
        return fail(RT_ERR_INVALID, "%s: rect = (%u, %u) .. (%u, %u) is not a rectangle inside the %u x %u image", who, rect[0], rect[1], rect[2], rect[3], ctx->width,
                    ctx->height);
    r[0] = rect ? rect[0] : 0u;
    r[1] = rect ? rect[1] : 0u;
    r[2] = rect ? rect[2] : ctx->width - 1u;
    r[3] = rect ? rect[3] : ctx->height - 1u;
    return RT_OK;
}

// What both entry points check before a device is looked for, and the rectangle they trace (the whole frame for NULL)
static int extents_args(const char *who, rt_ctx *ctx, const double cam[16], const uint32_t *rect, const void *out, bool dev_out, FrameArgs &fa, uint32_t r[4])
{
    if (!ctx || !cam || !out) return fail(RT_ERR_INVALID, "%s: null argument", who);
    if (dev_out && ((uintptr_t) out & 7u)) return fail(RT_ERR_INVALID, "%s: the output must be 8-byte aligned", who); // (the kernels' 64-bit atomics; a host array is only copied into)
    if (int rc = rect_args(who, ctx, rect, r)) return rc;
    return gbuffer_args(who, ctx, cam, fa);
}

// workgroups of one extents launch: four per CU, each striding over the tiles (rt_gbuffer.hip, extents_kernel)
static uint32_t extents_max_grid(const rt_ctx *ctx) { return ctx->wg_slots / 6u * 4u; }

// the launch behind both entry points; `who` names the one that called
static int extents_launch(const char *who, rt_ctx *ctx, const FrameArgs &fa, const uint32_t r[4], void *dev_out, hipStream_t stream)
{
    const hipError_t e = ctx->pixel_q->object_extents(&fa, ctx->d_obj, ctx->d_camx, ctx->d_camy, r, dev_out, extents_max_grid(ctx), &ctx->chunks[CULL_PIXELS], stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_object_extents(rt_ctx *ctx, const double cam[16], const uint32_t rect[4], rt_object_extent *dev_out, void *stream_, float *ms)
{
    static_assert(sizeof(rt_object_extent) == 40 && alignof(rt_object_extent) == 8, "rt_object_extent layout");
    hipStream_t stream = (hipStream_t) stream_;
    FrameArgs fa;
    uint32_t r[4];
    if (int rc = extents_args("rt_object_extents", ctx, cam, rect, dev_out, true, fa, r)) return rc;
    if (fa.n_obj == 0u) return RT_OK;
    if (int rc = timer_begin(ctx, stream, ms)) return rc;
    if (int rc = extents_launch("rt_object_extents", ctx, fa, r, dev_out, stream)) return rc;
    return timer_end(ctx, stream, ms);
}

extern "C" int rt_object_extents_host(rt_ctx *ctx, const double cam[16], const uint32_t rect[4], rt_object_extent *out_host, void *stream_)
{
    hipStream_t stream = (hipStream_t) stream_;
    FrameArgs fa;
    uint32_t r[4];
    if (int rc = extents_args("rt_object_extents_host", ctx, cam, rect, out_host, false, fa, r)) return rc;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream) RT_HIP(hipStreamIsCapturing(stream, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail(RT_ERR_INVALID, "rt_object_extents_host: the stream is capturing, and this call allocates and waits; capture rt_object_extents (device memory) instead");
    if (fa.n_obj == 0u) return RT_OK;
    if (int rc = ctx->ext.reserve(fa.n_obj, 8, sizeof(rt_object_extent))) return rc;
    if (int rc = extents_launch("rt_object_extents_host", ctx, fa, r, ctx->ext.out, stream)) return rc;
    RT_HIP(hipMemcpyAsync(out_host, ctx->ext.out, sizeof(rt_object_extent) * (size_t) fa.n_obj, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

// ---- ray queries (rt_rays.hip) ----------------------------------------------------------------------------
// A ray query reads the scene blob only: of the context's FrameArgs it takes the scene-layout words (the same in every context kind,
// supersampling included) and nothing of the frame.
static bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t pa = (uintptr_t) a, pb = (uintptr_t) b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

static int rays_ready(const char *who, rt_ctx *ctx)
{
    if (!ctx->stream_queries && rt_rays_lds_bytes_strict(&ctx->fa) > 160u * 1024u)
        return fail(RT_ERR_SCENE, "%s: scene needs %zu bytes of LDS per workgroup (limit 160 KiB)", who, rt_rays_lds_bytes_strict(&ctx->fa));
    return use_device(ctx);
}

// workgroups of one ray-query launch: four per CU (the kernels' registers allow three to four resident ones), fewer for few rays
static uint32_t rays_max_grid(const rt_ctx *ctx) { return ctx->wg_slots / 6u * 4u; }

// The ray entry points call the launchers rt_create decided on (rt_ctx::ray_q): the staged, the streamed, or -- RT_FLAG_STREAM_CULL_RAYS -- the culled ones
// (rt_stream_cull_rays.hip), which read the family's chunks.  The pixel queries have a decision of their own (rt_ctx::pixel_q).
static hipError_t trace_launch(rt_ctx *ctx, const void *dev_rays, uint32_t n, void *dev_hits, hipStream_t stream)
{
    return ctx->ray_q->trace_rays(&ctx->fa, ctx->d_obj, dev_rays, n, dev_hits, rays_max_grid(ctx), &ctx->chunks[CULL_RAYS], stream);
}

extern "C" int rt_trace_rays(rt_ctx *ctx, const rt_ray *dev_rays, uint32_t n, rt_hit *dev_hits, void *stream_, float *ms)
{
    static_assert(sizeof(rt_ray) == 48 && sizeof(rt_hit) == 48, "rt_ray / rt_hit layout");
    if (!ctx || !dev_rays || !dev_hits) return fail(RT_ERR_INVALID, "rt_trace_rays: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_trace_rays: n is 0");
    if (((uintptr_t) dev_rays | (uintptr_t) dev_hits) & 15u) return fail(RT_ERR_INVALID, "rt_trace_rays: rays and hits must be 16-byte aligned");
    if (ranges_overlap(dev_rays, sizeof(rt_ray) * (size_t) n, dev_hits, sizeof(rt_hit) * (size_t) n))
        return fail(RT_ERR_INVALID, "rt_trace_rays: the rays and the hits overlap");
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = rays_ready("rt_trace_rays", ctx)) return rc;
    if (int rc = timer_begin(ctx, stream, ms)) return rc;
    const hipError_t e = trace_launch(ctx, dev_rays, n, dev_hits, stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "ray-query kernel launch failed: %s", hipGetErrorString(e));
    return timer_end(ctx, stream, ms);
}

extern "C" int rt_occluded_rays(rt_ctx *ctx, const rt_ray *dev_rays, const double *dev_t_max, uint32_t n, int32_t *dev_blocked, void *stream_, float *ms)
{
    if (!ctx || !dev_rays || !dev_blocked) return fail(RT_ERR_INVALID, "rt_occluded_rays: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_occluded_rays: n is 0");
    if ((uintptr_t) dev_rays & 15u) return fail(RT_ERR_INVALID, "rt_occluded_rays: rays must be 16-byte aligned");
    if (((uintptr_t) dev_t_max & 7u) || ((uintptr_t) dev_blocked & 3u)) return fail(RT_ERR_INVALID, "rt_occluded_rays: t_max / flags are not aligned to their type");
    if (ranges_overlap(dev_rays, sizeof(rt_ray) * (size_t) n, dev_blocked, sizeof(int32_t) * (size_t) n) ||
        (dev_t_max && ranges_overlap(dev_t_max, sizeof(double) * (size_t) n, dev_blocked, sizeof(int32_t) * (size_t) n)))
        return fail(RT_ERR_INVALID, "rt_occluded_rays: the flags overlap the rays or t_max");
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = rays_ready("rt_occluded_rays", ctx)) return rc;
    if (int rc = timer_begin(ctx, stream, ms)) return rc;
    const hipError_t e = ctx->ray_q->occluded_rays(&ctx->fa, ctx->d_obj, dev_rays, dev_t_max, n, dev_blocked, rays_max_grid(ctx), &ctx->chunks[CULL_RAYS], stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "ray-query kernel launch failed: %s", hipGetErrorString(e));
    return timer_end(ctx, stream, ms);
}

extern "C" int rt_trace_rays_host(rt_ctx *ctx, const rt_ray *rays, uint32_t n, rt_hit *out, void *stream_)
{
    if (!ctx || !rays || !out) return fail(RT_ERR_INVALID, "rt_trace_rays_host: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_trace_rays_host: n is 0");
    if (ranges_overlap(rays, sizeof(rt_ray) * (size_t) n, out, sizeof(rt_hit) * (size_t) n)) return fail(RT_ERR_INVALID, "rt_trace_rays_host: the rays and the hits overlap");
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = rays_ready("rt_trace_rays_host", ctx)) return rc;
    if (int rc = ctx->rq.reserve(n, sizeof(rt_ray), sizeof(rt_hit))) return rc;
    RT_HIP(hipMemcpyAsync(ctx->rq.in, rays, sizeof(rt_ray) * (size_t) n, hipMemcpyHostToDevice, stream));
    const hipError_t e = trace_launch(ctx, ctx->rq.in, n, ctx->rq.out, stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "ray-query kernel launch failed: %s", hipGetErrorString(e));
    RT_HIP(hipMemcpyAsync(out, ctx->rq.out, sizeof(rt_hit) * (size_t) n, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

// ---- colour of caller-supplied rays (rt_shade_rays.hip) ----------------------------------------------------
// Like the ray queries it reads the scene (blob and lights) and nothing of the frame; always 4 x float32 per ray, whatever cfg.format.
static hipError_t shade_launch(rt_ctx *ctx, const void *dev_rays, uint32_t n, float *dev_rgba, void *dev_hits, hipStream_t stream)
{
    return ctx->ray_q->shade_rays(&ctx->fa, ctx->d_obj, ctx->d_light, dev_rays, n, dev_rgba, dev_hits, rays_max_grid(ctx), &ctx->chunks[CULL_RAYS], stream);
}

extern "C" int rt_shade_rays(rt_ctx *ctx, const rt_ray *dev_rays, uint32_t n, float *dev_rgba, rt_hit *dev_hits, void *stream_, float *ms)
{
    if (!ctx || !dev_rays || !dev_rgba) return fail(RT_ERR_INVALID, "rt_shade_rays: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_shade_rays: n is 0");
    if (((uintptr_t) dev_rays | (uintptr_t) dev_rgba | (uintptr_t) dev_hits) & 15u) return fail(RT_ERR_INVALID, "rt_shade_rays: rays, rgba and hits must be 16-byte aligned");
    const size_t ray_bytes = sizeof(rt_ray) * (size_t) n, px_bytes = 4 * sizeof(float) * (size_t) n, hit_bytes = sizeof(rt_hit) * (size_t) n;
    if (ranges_overlap(dev_rays, ray_bytes, dev_rgba, px_bytes)) return fail(RT_ERR_INVALID, "rt_shade_rays: the rays and the rgba output overlap");
    if (dev_hits && (ranges_overlap(dev_rays, ray_bytes, dev_hits, hit_bytes) || ranges_overlap(dev_rgba, px_bytes, dev_hits, hit_bytes)))
        return fail(RT_ERR_INVALID, "rt_shade_rays: the hits overlap the rays or the rgba output");
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = rays_ready("rt_shade_rays", ctx)) return rc;
    if (int rc = timer_begin(ctx, stream, ms)) return rc;
    const hipError_t e = shade_launch(ctx, dev_rays, n, dev_rgba, dev_hits, stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_shade_rays: kernel launch failed: %s", hipGetErrorString(e));
    return timer_end(ctx, stream, ms);
}

extern "C" int rt_shade_rays_host(rt_ctx *ctx, const rt_ray *rays, uint32_t n, float *rgba_out, void *stream_)
{
    if (!ctx || !rays || !rgba_out) return fail(RT_ERR_INVALID, "rt_shade_rays_host: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_shade_rays_host: n is 0");
    if (ranges_overlap(rays, sizeof(rt_ray) * (size_t) n, rgba_out, 4 * sizeof(float) * (size_t) n)) return fail(RT_ERR_INVALID, "rt_shade_rays_host: the rays and the rgba output overlap");
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = rays_ready("rt_shade_rays_host", ctx)) return rc;
    if (int rc = ctx->rq.reserve(n, sizeof(rt_ray), sizeof(rt_hit))) return rc;
    float *d_rgba = static_cast<float *>(ctx->rq.out.p); // (48 bytes per ray there, 16 needed)
    RT_HIP(hipMemcpyAsync(ctx->rq.in, rays, sizeof(rt_ray) * (size_t) n, hipMemcpyHostToDevice, stream));
    const hipError_t e = shade_launch(ctx, ctx->rq.in, n, d_rgba, nullptr, stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_shade_rays_host: kernel launch failed: %s", hipGetErrorString(e));
    RT_HIP(hipMemcpyAsync(rgba_out, d_rgba, 4 * sizeof(float) * (size_t) n, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

// ---- paths and the context's own primary rays (rt_paths.hip) ------------------------------------------------------
// Like the ray queries the path kernel reads the scene blob and nothing of the frame.
static hipError_t paths_launch(rt_ctx *ctx, const void *dev_rays, uint32_t n, uint32_t max_segments, void *dev_segments, void *dev_last, void *dev_ends, hipStream_t stream)
{
    return ctx->ray_q->trace_paths(&ctx->fa, ctx->d_obj, dev_rays, n, max_segments, dev_segments, dev_last, dev_ends, rays_max_grid(ctx), &ctx->chunks[CULL_RAYS], stream);
}

extern "C" int rt_trace_paths(rt_ctx *ctx, const rt_ray *dev_rays, uint32_t n, uint32_t max_segments, rt_hit *dev_segments, rt_hit *dev_last, rt_path_end *dev_ends,
                              void *stream_, float *ms)
{
    static_assert(sizeof(rt_path_end) == 16, "rt_path_end layout");
    if (!ctx || !dev_rays || !dev_ends) return fail(RT_ERR_INVALID, "rt_trace_paths: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_trace_paths: n is 0");
    if (max_segments > RT_PATH_MAX_SEGMENTS) return fail(RT_ERR_INVALID, "rt_trace_paths: max_segments %u exceeds %u", max_segments, RT_PATH_MAX_SEGMENTS);
    if (!dev_segments != (max_segments == 0u)) return fail(RT_ERR_INVALID, "rt_trace_paths: segments must be null if and only if max_segments is 0");
    if (((uintptr_t) dev_rays | (uintptr_t) dev_segments | (uintptr_t) dev_last | (uintptr_t) dev_ends) & 15u)
        return fail(RT_ERR_INVALID, "rt_trace_paths: rays, segments, last and ends must be 16-byte aligned");
    const struct { const void *p; size_t bytes; } range[4] = {{dev_rays, sizeof(rt_ray) * (size_t) n}, {dev_segments, sizeof(rt_hit) * (size_t) n * max_segments},
                                                              {dev_last, sizeof(rt_hit) * (size_t) n}, {dev_ends, sizeof(rt_path_end) * (size_t) n}};
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++)
            if (range[a].p && range[b].p && ranges_overlap(range[a].p, range[a].bytes, range[b].p, range[b].bytes))
                return fail(RT_ERR_INVALID, "rt_trace_paths: two of the rays, segments, last and ends ranges overlap");
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = rays_ready("rt_trace_paths", ctx)) return rc;
    if (int rc = timer_begin(ctx, stream, ms)) return rc;
    const hipError_t e = paths_launch(ctx, dev_rays, n, max_segments, dev_segments, dev_last, dev_ends, stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_trace_paths: kernel launch failed: %s", hipGetErrorString(e));
    return timer_end(ctx, stream, ms);
}

// the layout of ctx->pth for n rays and max_segments planes: every part a multiple of 16 bytes but the coordinates, which come last
struct PathStage {
    size_t rays, segments, last, ends, xy, bytes;
    PathStage(uint32_t n, uint32_t max_segments)
    {
        rays = 0;
        segments = rays + sizeof(rt_ray) * (size_t) n;
        last = segments + sizeof(rt_hit) * (size_t) n * max_segments;
        ends = last + sizeof(rt_hit) * (size_t) n;
        xy = ends + sizeof(rt_path_end) * (size_t) n;
        bytes = xy + sizeof(uint32_t) * 2 * (size_t) n;
    }
};

// the staged path kernel behind both blocking forms, and the copies back (last_out may be NULL)
static int paths_staged(const char *who, rt_ctx *ctx, const PathStage &st, uint32_t n, uint32_t max_segments, rt_hit *segments_out, rt_hit *last_out, rt_path_end *ends_out,
                        hipStream_t stream)
{
    unsigned char *d = ctx->pth.p;
    const hipError_t e = paths_launch(ctx, d + st.rays, n, max_segments, max_segments ? d + st.segments : nullptr, last_out ? d + st.last : nullptr, d + st.ends, stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    if (max_segments) RT_HIP(hipMemcpyAsync(segments_out, d + st.segments, st.last - st.segments, hipMemcpyDeviceToHost, stream));
    if (last_out) RT_HIP(hipMemcpyAsync(last_out, d + st.last, st.ends - st.last, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipMemcpyAsync(ends_out, d + st.ends, st.xy - st.ends, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

extern "C" int rt_trace_paths_host(rt_ctx *ctx, const rt_ray *rays, uint32_t n, uint32_t max_segments, rt_hit *segments_out, rt_hit *last_out, rt_path_end *ends_out,
                                   void *stream_)
{
    if (!ctx || !rays || !ends_out) return fail(RT_ERR_INVALID, "rt_trace_paths_host: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_trace_paths_host: n is 0");
    if (max_segments > RT_PATH_MAX_SEGMENTS) return fail(RT_ERR_INVALID, "rt_trace_paths_host: max_segments %u exceeds %u", max_segments, RT_PATH_MAX_SEGMENTS);
    if (!segments_out != (max_segments == 0u)) return fail(RT_ERR_INVALID, "rt_trace_paths_host: segments must be null if and only if max_segments is 0");
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = rays_ready("rt_trace_paths_host", ctx)) return rc;
    const PathStage st(n, max_segments);
    if (int rc = ctx->pth.reserve(st.bytes)) return rc;
    RT_HIP(hipMemcpyAsync(ctx->pth.p + st.rays, rays, sizeof(rt_ray) * (size_t) n, hipMemcpyHostToDevice, stream));
    return paths_staged("rt_trace_paths_host", ctx, st, n, max_segments, segments_out, last_out, ends_out, stream);
}

// workgroups of one primary-ray launch: the kernel only streams, a few workgroups per CU carry it
static uint32_t primary_max_grid(const rt_ctx *ctx) { return ctx->wg_slots / 6u * 8u; }

extern "C" int rt_primary_rays(rt_ctx *ctx, const double cam[16], const uint32_t rect[4], rt_ray *dev_rays, void *stream_, float *ms)
{
    if (!ctx || !cam || !dev_rays) return fail(RT_ERR_INVALID, "rt_primary_rays: null argument");
    if ((uintptr_t) dev_rays & 15u) return fail(RT_ERR_INVALID, "rt_primary_rays: the rays must be 16-byte aligned");
    hipStream_t stream = (hipStream_t) stream_;
    FrameArgs fa;
    uint32_t r[4];
    if (int rc = rect_args("rt_primary_rays", ctx, rect, r)) return rc;
    if (int rc = gbuffer_args("rt_primary_rays", ctx, cam, fa)) return rc;
    if (int rc = timer_begin(ctx, stream, ms)) return rc;
    const hipError_t e = ctx->kern->primary_rays(&fa, ctx->d_camx, ctx->d_camy, r, nullptr, 0u, dev_rays, primary_max_grid(ctx), stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_primary_rays: kernel launch failed: %s", hipGetErrorString(e));
    return timer_end(ctx, stream, ms);
}

extern "C" int rt_pick_paths(rt_ctx *ctx, const double cam[16], const uint32_t *xy, uint32_t n, uint32_t max_segments, rt_hit *segments_host, rt_path_end *ends_host,
                             void *stream_)
{
    if (!ctx || !cam || !xy || !ends_host) return fail(RT_ERR_INVALID, "rt_pick_paths: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_pick_paths: n is 0");
    if (max_segments > RT_PATH_MAX_SEGMENTS) return fail(RT_ERR_INVALID, "rt_pick_paths: max_segments %u exceeds %u", max_segments, RT_PATH_MAX_SEGMENTS);
    if (!segments_host != (max_segments == 0u)) return fail(RT_ERR_INVALID, "rt_pick_paths: segments must be null if and only if max_segments is 0");
    if (int rc = pixels_inside("rt_pick_paths", ctx, xy, n)) return rc;
    hipStream_t stream = (hipStream_t) stream_;
    FrameArgs fa;
    if (int rc = gbuffer_args("rt_pick_paths", ctx, cam, fa)) return rc;
    if (int rc = rays_ready("rt_pick_paths", ctx)) return rc;
    const PathStage st(n, max_segments);
    if (int rc = ctx->pth.reserve(st.bytes)) return rc;
    unsigned char *d = ctx->pth.p;
    RT_HIP(hipMemcpyAsync(d + st.xy, xy, sizeof(uint32_t) * 2 * (size_t) n, hipMemcpyHostToDevice, stream));
    const hipError_t e = ctx->kern->primary_rays(&fa, ctx->d_camx, ctx->d_camy, nullptr, reinterpret_cast<const uint32_t *>(d + st.xy), n, d + st.rays, primary_max_grid(ctx), stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_pick_paths: kernel launch failed: %s", hipGetErrorString(e));
    return paths_staged("rt_pick_paths", ctx, st, n, max_segments, segments_host, nullptr, ends_host, stream);
}

// ---- scene updates (rt_set_scene.hip) -----------------------------------------------------------------------
static const char *reject_text(uint32_t reason)
{
    switch (reason) {
    case RT_SCENE_REJECT_CLASS: return "the object would move to another class table";
    case RT_SCENE_REJECT_BOUND: return "the unit sphere would gain or lose its bounding radius";
    case RT_SCENE_REJECT_MIRROR: return "the scene would gain its first mirror or lose its last (object)";
    case RT_SCENE_REJECT_CUBIC: return "a coefficient of the degree-3 object differs";
    case RT_SCENE_REJECT_LIGHT: return "the light's table flags would change (|direction|^2 against 1e-7, or finite colours / albedos)";
    default: return "unknown reason";
    }
}

// Copy `bytes` from device memory behind everything the context has enqueued, and wait for that alone: the copy runs on the stream of
// the context's last call (frames and updates of a context are ordered on it), so no other stream of the device is stalled.  Refused
// while that stream is capturing -- nothing can be waited for inside a capture.
static int read_behind_last_call(const char *who, rt_ctx *ctx, void *dst, const void *src, size_t bytes, void *dst2 = nullptr, const void *src2 = nullptr, size_t bytes2 = 0)
{
    if (int rc = use_device(ctx)) return rc;
    hipStream_t stream = ctx->last_stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream) RT_HIP(hipStreamIsCapturing(stream, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(RT_ERR_INVALID, "%s: the context's stream is capturing; end the capture first", who);
    RT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
    if (bytes2) RT_HIP(hipMemcpyAsync(dst2, src2, bytes2, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

static int set_scene_check(const char *who, const rt_ctx *ctx, const rt_scene_update *u)
{
    if (!u->coefs && !u->reflection && !u->albedo && !u->light_p && !u->light_color) return fail(RT_ERR_INVALID, "%s: all five arrays are null", who);
    if (((uintptr_t) u->coefs | (uintptr_t) u->light_p) & 7u) return fail(RT_ERR_INVALID, "%s: coefs / light_p must be 8-byte aligned", who);
    if (((uintptr_t) u->reflection | (uintptr_t) u->albedo | (uintptr_t) u->light_color) & 3u)
        return fail(RT_ERR_INVALID, "%s: reflection / albedo / light_color must be 4-byte aligned", who);
    if (ctx->fa.n_obj == 0u && (u->coefs || u->reflection || u->albedo)) return fail(RT_ERR_INVALID, "%s: an object array for a scene without objects", who);
    if (ctx->fa.n_lights == 0u && (u->light_p || u->light_color)) return fail(RT_ERR_INVALID, "%s: a light array for a scene without lights", who);
    return RT_OK;
}

// enqueue the kernel on `stream`, in the context's frame order (order_begin / order_end, as a render)
static int set_scene_enqueue(const char *who, rt_ctx *ctx, const rt_scene_update *dev, hipStream_t stream)
{
    if (int rc = use_device(ctx)) return rc;
    bool capturing = false;
    if (int rc = order_begin(who, ctx, stream, &capturing)) return rc;
    const FrameArgs &fa = ctx->fa;
    SetSceneArgs a{};
    a.blob = reinterpret_cast<unsigned char *>(ctx->d_obj.p);
    a.lights = ctx->d_light;
    a.status = ctx->d_ss_status;
    a.coefs = dev->coefs;
    a.reflection = dev->reflection;
    a.albedo = dev->albedo;
    a.light_p = dev->light_p;
    a.light_color = dev->light_color;
    a.n_obj = fa.n_obj;
    a.n_lights = fa.n_lights;
    a.n_us = fa.n_us;
    a.n_gq = fa.n_gq;
    a.n_lin = fa.n_lin;
    a.off_us = fa.off_us;
    a.off_gq = fa.off_gq;
    a.off_lin = fa.off_lin;
    a.off_mat = fa.off_mat;
    a.has_mirror = fa.has_mirror;
    a.n_chunks = ctx->cull[CULL_FRAME] ? ctx->n_chunks : 0u; // (the chunk bounds follow the rebuilt entries; the slots keep their objects: only rt_reorder_scene moves an entry)
    a.bounds = ctx->cull[CULL_FRAME] ? ctx->d_bounds.p : nullptr;
    hipError_t e = rt_launch_set_scene(&a, stream);
    if (e == hipSuccess && ctx->groups) e = rt_launch_group_bounds(ctx->d_bounds.p, ctx->n_chunks, ctx->d_groups.p, stream); // (a refused update: the same bytes again)
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return order_end(ctx, stream, capturing);
}

extern "C" int rt_set_scene(rt_ctx *ctx, const rt_scene_update *dev, void *stream)
{
    if (!ctx || !dev) return fail(RT_ERR_INVALID, "rt_set_scene: null argument");
    if (int rc = set_scene_check("rt_set_scene", ctx, dev)) return rc;
    return set_scene_enqueue("rt_set_scene", ctx, dev, (hipStream_t) stream);
}

extern "C" int rt_set_scene_host(rt_ctx *ctx, const rt_scene_update *host, void *stream_)
{
    if (!ctx || !host) return fail(RT_ERR_INVALID, "rt_set_scene_host: null argument");
    if (int rc = set_scene_check("rt_set_scene_host", ctx, host)) return rc;
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = use_device(ctx)) return rc;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream) RT_HIP(hipStreamIsCapturing(stream, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail(RT_ERR_INVALID, "rt_set_scene_host: the stream is capturing, and this call allocates and waits; capture rt_set_scene (device arrays) instead");
    // staging: the five arrays back to back, the FP64 ones first (n_objects and n_lights are fixed, so one allocation serves every call)
    const size_t no = ctx->fa.n_obj, nl = ctx->fa.n_lights;
    const size_t b_coefs = sizeof(double) * RT_NCOEF * no, b_lp = sizeof(double) * 3 * nl, b_refl = sizeof(float) * no, b_alb = sizeof(float) * 3 * no,
                 b_lc = sizeof(float) * 3 * nl;
    if (!ctx->d_ss_stage) RT_HIP(ctx->d_ss_stage.alloc(b_coefs + b_lp + b_refl + b_alb + b_lc));
    unsigned char *p = ctx->d_ss_stage;
    rt_scene_update dev{};
    auto put = [&](const void *src, size_t bytes) -> const void * {
        unsigned char *dst = p;
        p += bytes;
        if (!src) return nullptr;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) == hipSuccess ? dst : nullptr;
    };
    dev.coefs = (const double *) put(host->coefs, b_coefs);
    dev.light_p = (const double *) put(host->light_p, b_lp);
    dev.reflection = (const float *) put(host->reflection, b_refl);
    dev.albedo = (const float *) put(host->albedo, b_alb);
    dev.light_color = (const float *) put(host->light_color, b_lc);
    if ((!dev.coefs != !host->coefs) || (!dev.light_p != !host->light_p) || (!dev.reflection != !host->reflection) || (!dev.albedo != !host->albedo) ||
        (!dev.light_color != !host->light_color))
        return fail(RT_ERR_DEVICE, "rt_set_scene_host: hipMemcpyAsync failed: %s", hipGetErrorString(hipGetLastError()));
    if (int rc = set_scene_enqueue("rt_set_scene_host", ctx, &dev, stream)) return rc;
    SetSceneStatus st{};
    RT_HIP(hipMemcpyAsync(&st, ctx->d_ss_status, sizeof(st), hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    if (st.last == 2u)
        return fail(RT_ERR_SCENE, "rt_set_scene_host: update rejected, nothing was written: reason %u at index %u: %s", st.reason, st.index, reject_text(st.reason));
    return RT_OK;
}

// Re-sort the unit-sphere table the device holds now into the order rt_create would choose for it, and rebuild the chunk bounds: kernels only, in the
// context's frame order (order_begin / order_end, as rt_set_scene), every launch decided at rt_create.  A context whose decision is false enqueues nothing.
extern "C" int rt_reorder_scene(rt_ctx *ctx, void *stream_)
{
    if (!ctx) return fail(RT_ERR_INVALID, "rt_reorder_scene: null argument");
    if (!ctx->reorder) return RT_OK;
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = use_device(ctx)) return rc;
    bool capturing = false;
    if (int rc = order_begin("rt_reorder_scene", ctx, stream, &capturing)) return rc;
    const FrameArgs &fa = ctx->fa;
    unsigned char *blob = reinterpret_cast<unsigned char *>(ctx->d_obj.p);
    hipError_t e = rt_launch_reorder_scene(blob + fa.off_us, fa.n_us, fa.n_obj, ctx->d_bounds.p, ctx->d_reorder_work.p, ctx->reorder_max_grid, stream);
    if (e == hipSuccess && ctx->groups) e = rt_launch_group_bounds(ctx->d_bounds.p, ctx->n_chunks, ctx->d_groups.p, stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_reorder_scene: kernel launch failed: %s", hipGetErrorString(e));
    return order_end(ctx, stream, capturing);
}

extern "C" int rt_get_stream_cull_reorder(const rt_ctx *ctx, uint32_t *on)
{
    if (!ctx || !on) return fail(RT_ERR_INVALID, "rt_get_stream_cull_reorder: null argument");
    *on = ctx->reorder ? 1u : 0u;
    return RT_OK;
}

extern "C" int rt_set_scene_status(rt_ctx *ctx, uint64_t *applied, uint64_t *rejected, uint32_t *reason, uint32_t *index)
{
    if (!ctx) return fail(RT_ERR_INVALID, "rt_set_scene_status: null argument");
    SetSceneStatus st{};
    if (int rc = read_behind_last_call("rt_set_scene_status", ctx, &st, ctx->d_ss_status, sizeof(st))) return rc;
    if (applied) *applied = st.applied;
    if (rejected) *rejected = st.rejected;
    if (reason) *reason = st.reason;
    if (index) *index = st.index;
    return RT_OK;
}

extern "C" int rt_debug_scene_blob(rt_ctx *ctx, void *out, size_t cap, size_t *bytes)
{
    if (!ctx || !bytes) return fail(RT_ERR_INVALID, "rt_debug_scene_blob: null argument");
    const size_t light_bytes = (sizeof(DevLight) + sizeof(LightK)) * (size_t) ctx->fa.n_lights, need = (size_t) ctx->fa.scene_bytes + light_bytes;
    *bytes = need;
    if (!out) return RT_OK;
    if (cap < need) return fail(RT_ERR_INVALID, "rt_debug_scene_blob: %zu bytes offered, the scene takes %zu", cap, need);
    return read_behind_last_call("rt_debug_scene_blob", ctx, out, ctx->d_obj, ctx->fa.scene_bytes, (unsigned char *) out + ctx->fa.scene_bytes, ctx->d_light, light_bytes);
}

extern "C" int rt_local_rows(const rt_ctx *ctx, uint32_t *n_rows)
{
    if (!ctx || !n_rows) return fail(RT_ERR_INVALID, "rt_local_rows: null argument");
    *n_rows = ctx->local_rows;
    return RT_OK;
}

extern "C" int rt_max_local_rows(const rt_ctx *ctx, uint32_t *n_rows)
{
    if (!ctx || !n_rows) return fail(RT_ERR_INVALID, "rt_max_local_rows: null argument");
    *n_rows = ctx->max_local_rows;
    return RT_OK;
}

extern "C" int rt_row_map(const rt_ctx *ctx, uint32_t *rows)
{
    if (!ctx || !rows) return fail(RT_ERR_INVALID, "rt_row_map: null argument");
    const uint32_t B = ctx->cfg.band_rows, W = ctx->cfg.world, R = ctx->cfg.rank;
    for (uint32_t lr = 0; lr < ctx->local_rows; lr++) {
        uint32_t b = lr / B;
        rows[lr] = (b * W + R) * B + (lr - b * B);
    }
    return RT_OK;
}

extern "C" size_t rt_pixel_bytes(const rt_ctx *ctx) { return ctx ? ctx->pixel_bytes : 0; }

extern "C" void *rt_device_fb(rt_ctx *ctx) { return ctx ? ctx->d_fb.p : nullptr; }

extern "C" int rt_download(rt_ctx *ctx, void *host_dst, size_t bytes)
{
    if (!ctx || !host_dst) return fail(RT_ERR_INVALID, "rt_download: null argument");
    const size_t have = (size_t) ctx->local_rows * ctx->width * ctx->pixel_bytes;
    if (bytes > have) return fail(RT_ERR_INVALID, "rt_download: %zu bytes requested, framebuffer holds %zu", bytes, have);
    return read_synced(ctx, host_dst, ctx->d_fb, bytes);
}

extern "C" int rt_assemble(rt_ctx *ctx, const void *gathered, void *full, void *stream)
{
    if (!ctx || !gathered || !full) return fail(RT_ERR_INVALID, "rt_assemble: null argument");
    hipError_t e = rt_launch_assemble_strict(gathered, full, ctx->width, ctx->height, ctx->cfg.world, ctx->cfg.band_rows,
                                             ctx->max_local_rows, ctx->cfg.format == RT_FMT_RGBA8, (hipStream_t) stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "assemble launch failed: %s", hipGetErrorString(e));
    return RT_OK;
}

// ---- planes and records of several ranks (rt_planes.hip) ----------------------------------------------------
// rt_assemble for planes that are not frames: elements of 4, 8 or 16 bytes (the G-buffer's object, t and normal planes), rank q's slot at
// gathered + q * slot_stride_bytes.  Everything is decided from the arguments and the context's geometry before a device is looked for.
extern "C" int rt_assemble_planes(rt_ctx *ctx, const void *gathered, size_t slot_stride_bytes, void *full, uint32_t elem_bytes, void *stream)
{
    if (!ctx || !gathered || !full) return fail(RT_ERR_INVALID, "rt_assemble_planes: null argument");
    if (elem_bytes != 4u && elem_bytes != 8u && elem_bytes != 16u) return fail(RT_ERR_INVALID, "rt_assemble_planes: elem_bytes is %u (4, 8 or 16)", elem_bytes);
    if (ctx->ssaa > 1u || ctx->adaptive)
        return fail(RT_ERR_INVALID, "rt_assemble_planes: not available for contexts created with RT_FLAG_SSAA2 / RT_FLAG_SSAA4 / RT_FLAG_SSAA_ADAPTIVE");
    const size_t slot = (size_t) ctx->max_local_rows * ctx->width * elem_bytes, full_bytes = (size_t) ctx->height * ctx->width * elem_bytes;
    if (slot_stride_bytes < slot || slot_stride_bytes % elem_bytes)
        return fail(RT_ERR_INVALID, "rt_assemble_planes: a slot stride of %zu bytes (at least one slot of %zu bytes, and a multiple of elem_bytes = %u)", slot_stride_bytes, slot,
                    elem_bytes);
    if (((uintptr_t) gathered | (uintptr_t) full) & (elem_bytes - 1u)) return fail(RT_ERR_INVALID, "rt_assemble_planes: gathered and full must be aligned to elem_bytes = %u", elem_bytes);
    if (ranges_overlap(gathered, slot_stride_bytes * (ctx->cfg.world - 1u) + slot, full, full_bytes)) return fail(RT_ERR_INVALID, "rt_assemble_planes: full overlaps gathered");
    if (int rc = use_device(ctx)) return rc;
    const hipError_t e = rt_launch_assemble_planes(gathered, slot_stride_bytes / elem_bytes, full, ctx->width, ctx->height, ctx->cfg.world, ctx->cfg.band_rows, elem_bytes,
                                                   (hipStream_t) stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_assemble_planes: kernel launch failed: %s", hipGetErrorString(e));
    return RT_OK;
}

// The records of n_parts ranks (or of anything else that reduces the same way) into one: sum / min / max, the identities included.
extern "C" int rt_merge_object_extents(rt_ctx *ctx, const rt_object_extent *dev_parts, uint32_t n_parts, rt_object_extent *dev_out, void *stream)
{
    if (!ctx || !dev_parts || !dev_out) return fail(RT_ERR_INVALID, "rt_merge_object_extents: null argument");
    if (n_parts == 0u) return fail(RT_ERR_INVALID, "rt_merge_object_extents: n_parts is 0");
    if (((uintptr_t) dev_parts | (uintptr_t) dev_out) & 7u) return fail(RT_ERR_INVALID, "rt_merge_object_extents: the records must be 8-byte aligned");
    const size_t out_bytes = sizeof(rt_object_extent) * (size_t) ctx->fa.n_obj;
    if (out_bytes && ranges_overlap(dev_parts, out_bytes * n_parts, dev_out, out_bytes)) return fail(RT_ERR_INVALID, "rt_merge_object_extents: the output overlaps the parts");
    if (ctx->fa.n_obj == 0u) return RT_OK;
    if (int rc = use_device(ctx)) return rc;
    const hipError_t e = rt_launch_merge_extents(dev_parts, n_parts, ctx->fa.n_obj, dev_out, (hipStream_t) stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_merge_object_extents: kernel launch failed: %s", hipGetErrorString(e));
    return RT_OK;
}

// ---- sorting caller-supplied rays (rt_sort_rays.hip) ----------------------------------------------------------
// No scene state: the context selects the device, the grid bound and the error conventions, as in rt_assemble_planes.  Everything is decided
// from the arguments before a device is looked for.
extern "C" size_t rt_sort_rays_work_bytes(uint32_t n) { return rt_sort_rays_work_size(n); }

extern "C" int rt_sort_rays(rt_ctx *ctx, const rt_ray *dev_rays, uint32_t n, rt_ray *dev_sorted, uint32_t *dev_perm, uint32_t *dev_keys, void *dev_work, size_t work_bytes,
                            void *stream_, float *ms)
{
    if (!ctx || !dev_rays || !dev_perm || !dev_work) return fail(RT_ERR_INVALID, "rt_sort_rays: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_sort_rays: n is 0");
    if (((uintptr_t) dev_rays | (uintptr_t) dev_sorted) & 15u) return fail(RT_ERR_INVALID, "rt_sort_rays: rays and sorted rays must be 16-byte aligned");
    if (((uintptr_t) dev_perm | (uintptr_t) dev_keys) & 3u) return fail(RT_ERR_INVALID, "rt_sort_rays: perm / keys are not aligned to their type");
    const size_t need = rt_sort_rays_work_size(n);
    if (work_bytes < need) return fail(RT_ERR_INVALID, "rt_sort_rays: %zu bytes of work space offered, %u rays take %zu (rt_sort_rays_work_bytes)", work_bytes, n, need);
    const struct { const void *p; size_t bytes; } range[5] = {{dev_rays, sizeof(rt_ray) * (size_t) n}, {dev_sorted, sizeof(rt_ray) * (size_t) n}, {dev_perm, sizeof(uint32_t) * (size_t) n},
                                                             {dev_keys, sizeof(uint32_t) * (size_t) n}, {dev_work, work_bytes}};
    for (int a = 0; a < 5; a++)
        for (int b = a + 1; b < 5; b++)
            if (range[a].p && range[b].p && ranges_overlap(range[a].p, range[a].bytes, range[b].p, range[b].bytes))
                return fail(RT_ERR_INVALID, "rt_sort_rays: two of the rays, sorted rays, perm, keys and work space ranges overlap");
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = use_device(ctx)) return rc;
    if (int rc = timer_begin(ctx, stream, ms)) return rc;
    const hipError_t e = rt_launch_sort_rays(dev_rays, n, dev_sorted, dev_perm, dev_keys, dev_work, rays_max_grid(ctx), stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_sort_rays: kernel launch failed: %s", hipGetErrorString(e));
    return timer_end(ctx, stream, ms);
}

extern "C" int rt_permute(rt_ctx *ctx, const uint32_t *dev_perm, uint32_t n, const void *dev_src, void *dev_dst, uint32_t elem_bytes, uint32_t planes, int scatter,
                          void *stream_, float *ms)
{
    if (!ctx || !dev_perm || !dev_src || !dev_dst) return fail(RT_ERR_INVALID, "rt_permute: null argument");
    if (n == 0) return fail(RT_ERR_INVALID, "rt_permute: n is 0");
    if (elem_bytes == 0u || (elem_bytes & 3u) || elem_bytes > 256u) return fail(RT_ERR_INVALID, "rt_permute: elem_bytes is %u (a multiple of 4, at most 256)", elem_bytes);
    if (planes == 0u) return fail(RT_ERR_INVALID, "rt_permute: planes is 0");
    if (((uintptr_t) dev_perm | (uintptr_t) dev_src | (uintptr_t) dev_dst) & 3u) return fail(RT_ERR_INVALID, "rt_permute: perm, src and dst must be 4-byte aligned");
    const size_t bytes = (size_t) n * elem_bytes * planes;
    if (ranges_overlap(dev_src, bytes, dev_dst, bytes)) return fail(RT_ERR_INVALID, "rt_permute: src overlaps dst");
    if (ranges_overlap(dev_perm, sizeof(uint32_t) * (size_t) n, dev_dst, bytes)) return fail(RT_ERR_INVALID, "rt_permute: perm overlaps dst");
    hipStream_t stream = (hipStream_t) stream_;
    if (int rc = use_device(ctx)) return rc;
    if (int rc = timer_begin(ctx, stream, ms)) return rc;
    const hipError_t e = rt_launch_permute(dev_perm, n, dev_src, dev_dst, elem_bytes, planes, scatter, rays_max_grid(ctx), stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "rt_permute: kernel launch failed: %s", hipGetErrorString(e));
    return timer_end(ctx, stream, ms);
}

extern "C" size_t rt_sparse_bytes(uint32_t capacity_tiles)
{
    return ((size_t) ((4u + capacity_tiles + 3u) & ~3u) + (size_t) capacity_tiles * 256u) * sizeof(uint32_t);
}

extern "C" size_t rt_sparse_msg_bytes(uint32_t format, uint32_t capacity_tiles)
{
    if (format == RT_FMT_RGBA8) return rt_sparse_bytes(capacity_tiles);
    if (format == RT_FMT_RGBA32F) return ((size_t) ((4u + capacity_tiles + 3u) & ~3u) + (size_t) capacity_tiles * 1024u) * sizeof(uint32_t);
    return 0;
}

extern "C" int rt_pack_sparse(rt_ctx *ctx, const void *dev_fb, void *dev_msg, uint32_t capacity_tiles, void *stream)
{
    if (!ctx || !dev_msg) return fail(RT_ERR_INVALID, "rt_pack_sparse: null argument");
    const BgPixel bg = bg_pixel(ctx);
    hipError_t e = rt_launch_pack_sparse_strict(dev_fb ? dev_fb : ctx->d_fb.p, dev_msg, ctx->width, ctx->local_rows, bg.w, capacity_tiles,
                                                ctx->cfg.format == RT_FMT_RGBA8, (hipStream_t) stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "pack launch failed: %s", hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_assemble_sparse(rt_ctx *ctx, const void *gathered, uint32_t capacity_tiles, void *full, void *stream)
{
    if (!ctx || !gathered || !full) return fail(RT_ERR_INVALID, "rt_assemble_sparse: null argument");
    const BgPixel bg = bg_pixel(ctx);
    hipError_t e = rt_launch_assemble_sparse_strict(gathered, full, ctx->width, ctx->height, ctx->cfg.world, ctx->cfg.band_rows, bg.w, capacity_tiles,
                                                    nullptr, 0, 0, ctx->cfg.format == RT_FMT_RGBA8, (hipStream_t) stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "sparse assemble launch failed: %s", hipGetErrorString(e));
    return RT_OK;
}

// tiles of the rank with the most rows: the stamps of the incremental assembly are [world][max_tiles]
static size_t sparse_max_tiles(const rt_ctx *ctx) { return (size_t) ((ctx->width + 15u) / 16u) * ((ctx->max_local_rows + 15u) / 16u); }

extern "C" size_t rt_sparse_stamp_bytes(rt_ctx *ctx)
{
    if (!ctx) return 0;
    return sizeof(uint32_t) * (size_t) ctx->cfg.world * sparse_max_tiles(ctx);
}

extern "C" int rt_assemble_sparse_incremental(rt_ctx *ctx, const void *gathered, uint32_t capacity_tiles, void *full, void *stamps, uint32_t frame_tag,
                                              void *stream)
{
    if (!ctx || !gathered || !full || !stamps) return fail(RT_ERR_INVALID, "rt_assemble_sparse_incremental: null argument");
    const uint32_t max_tiles = (uint32_t) sparse_max_tiles(ctx);
    const BgPixel bg = bg_pixel(ctx);
    hipError_t e = rt_launch_assemble_sparse_strict(gathered, full, ctx->width, ctx->height, ctx->cfg.world, ctx->cfg.band_rows, bg.w, capacity_tiles,
                                                    stamps, max_tiles, frame_tag, ctx->cfg.format == RT_FMT_RGBA8, (hipStream_t) stream);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, "sparse assemble launch failed: %s", hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_set_ssaa_threshold(rt_ctx *ctx, float tau)
{
    if (!ctx) return fail(RT_ERR_INVALID, "rt_set_ssaa_threshold: null argument");
    if (!ctx->adaptive) return fail(RT_ERR_INVALID, "rt_set_ssaa_threshold: the context was not created with RT_FLAG_SSAA_ADAPTIVE");
    if (std::isnan(tau)) return fail(RT_ERR_INVALID, "rt_set_ssaa_threshold: tau is NaN");
    ctx->tau = tau;
    return RT_OK;
}

extern "C" int rt_set_ssaa_geometry(rt_ctx *ctx, float min_cos)
{
    if (!ctx) return fail(RT_ERR_INVALID, "rt_set_ssaa_geometry: null argument");
    if (!ctx->geometry) return fail(RT_ERR_INVALID, "rt_set_ssaa_geometry: the context was not created with RT_FLAG_SSAA_GEOMETRY");
    if (std::isnan(min_cos)) return fail(RT_ERR_INVALID, "rt_set_ssaa_geometry: min_cos is NaN");
    ctx->min_cos = min_cos;
    return RT_OK;
}

extern "C" int rt_get_ssaa_refined(rt_ctx *ctx, uint64_t *pixels)
{
    if (!ctx || !pixels) return fail(RT_ERR_INVALID, "rt_get_ssaa_refined: null argument");
    if (!ctx->adaptive) return fail(RT_ERR_INVALID, "rt_get_ssaa_refined: the context was not created with RT_FLAG_SSAA_ADAPTIVE");
    uint32_t n = 0;
    if (int rc = read_synced(ctx, &n, ctx->d_list + (size_t) ctx->local_rows * ctx->width, sizeof(n))) return rc;
    *pixels = n;
    return RT_OK;
}

extern "C" int rt_get_streamed_queries(const rt_ctx *ctx, uint32_t *streamed)
{
    if (!ctx || !streamed) return fail(RT_ERR_INVALID, "rt_get_streamed_queries: null argument");
    *streamed = ctx->stream_queries ? 1u : 0u;
    return RT_OK;
}

extern "C" int rt_get_streamed_adaptive(const rt_ctx *ctx, uint32_t *streamed)
{
    if (!ctx || !streamed) return fail(RT_ERR_INVALID, "rt_get_streamed_adaptive: null argument");
    *streamed = ctx->stream_adaptive ? 1u : 0u;
    return RT_OK;
}

// The getter and the debug reader of a culling family (cull_family[] holds their names and what the refusal says)
static int get_cull(CullFamily f, const rt_ctx *ctx, uint32_t *on)
{
    if (!ctx || !on) return fail(RT_ERR_INVALID, "%s: null argument", cull_family[f].get);
    *on = ctx->cull[f] ? 1u : 0u;
    return RT_OK;
}

static int debug_cull(CullFamily f, rt_ctx *ctx, uint64_t out[8])
{
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "work words");
    const char *who = cull_family[f].debug;
    if (!ctx || !out) return fail(RT_ERR_INVALID, "%s: null argument", who);
    if (!ctx->chunks[f].stats)
        return fail(RT_ERR_INVALID, "%s: the context keeps no work words (they exist where %s says 1%s)", who, cull_family[f].get, cull_family[f].also);
    return read_behind_last_call(who, ctx, out, ctx->chunks[f].stats, sizeof(uint64_t) * 8);
}

extern "C" int rt_get_stream_cull(const rt_ctx *ctx, uint32_t *on) { return get_cull(CULL_FRAME, ctx, on); }
extern "C" int rt_debug_stream_cull(rt_ctx *ctx, uint64_t out[8]) { return debug_cull(CULL_FRAME, ctx, out); }
extern "C" int rt_get_stream_cull_adaptive(const rt_ctx *ctx, uint32_t *on) { return get_cull(CULL_ADAPTIVE, ctx, on); }
extern "C" int rt_debug_stream_cull_adaptive(rt_ctx *ctx, uint64_t out[8]) { return debug_cull(CULL_ADAPTIVE, ctx, out); }
extern "C" int rt_get_stream_cull_bounce(const rt_ctx *ctx, uint32_t *on) { return get_cull(CULL_BOUNCE, ctx, on); }
extern "C" int rt_debug_stream_cull_bounce(rt_ctx *ctx, uint64_t out[8]) { return debug_cull(CULL_BOUNCE, ctx, out); }
extern "C" int rt_get_stream_cull_rays(const rt_ctx *ctx, uint32_t *on) { return get_cull(CULL_RAYS, ctx, on); }
extern "C" int rt_debug_stream_cull_rays(rt_ctx *ctx, uint64_t out[8]) { return debug_cull(CULL_RAYS, ctx, out); }
extern "C" int rt_get_stream_cull_pixels(const rt_ctx *ctx, uint32_t *on) { return get_cull(CULL_PIXELS, ctx, on); }
extern "C" int rt_debug_stream_cull_pixels(rt_ctx *ctx, uint64_t out[8]) { return debug_cull(CULL_PIXELS, ctx, out); }

extern "C" int rt_debug_stream_bounds(rt_ctx *ctx, void *out, size_t cap, size_t *bytes)
{
    if (!ctx || !bytes) return fail(RT_ERR_INVALID, "rt_debug_stream_bounds: null argument");
    const size_t need = ctx->cull[CULL_FRAME] ? sizeof(UsEntry) * (size_t) ctx->n_chunks : 0u;
    *bytes = need;
    if (!out || !need) return RT_OK;
    if (cap < need) return fail(RT_ERR_INVALID, "rt_debug_stream_bounds: %zu bytes offered, the bounds take %zu", cap, need);
    return read_behind_last_call("rt_debug_stream_bounds", ctx, out, ctx->d_bounds, need);
}

// RT_FLAG_STREAM_CULL_GROUPS: the decision, the group work words, the group bounds as the device holds them
extern "C" int rt_get_stream_groups(const rt_ctx *ctx, uint32_t *on)
{
    if (!ctx || !on) return fail(RT_ERR_INVALID, "rt_get_stream_groups: null argument");
    *on = ctx->groups ? 1u : 0u;
    return RT_OK;
}

extern "C" int rt_debug_stream_groups(rt_ctx *ctx, uint64_t out[8])
{
    if (!ctx || !out) return fail(RT_ERR_INVALID, "rt_debug_stream_groups: null argument");
    if (!ctx->group_tables.stats)
        return fail(RT_ERR_INVALID, "rt_debug_stream_groups: the context keeps no work words (they exist where rt_get_stream_groups says 1%s)", STATS_SET);
    return read_behind_last_call("rt_debug_stream_groups", ctx, out, ctx->group_tables.stats, sizeof(uint64_t) * 8);
}

extern "C" int rt_debug_stream_group_bounds(rt_ctx *ctx, void *out, size_t cap, size_t *bytes)
{
    if (!ctx || !bytes) return fail(RT_ERR_INVALID, "rt_debug_stream_group_bounds: null argument");
    const size_t need = ctx->groups ? sizeof(UsEntry) * (size_t) ctx->n_groups : 0u;
    *bytes = need;
    if (!out || !need) return RT_OK;
    if (cap < need) return fail(RT_ERR_INVALID, "rt_debug_stream_group_bounds: %zu bytes offered, the group bounds take %zu", cap, need);
    return read_behind_last_call("rt_debug_stream_group_bounds", ctx, out, ctx->d_groups, need);
}

extern "C" int rt_get_streamed(const rt_ctx *ctx, uint32_t *streamed)
{
    if (!ctx || !streamed) return fail(RT_ERR_INVALID, "rt_get_streamed: null argument");
    *streamed = ctx->streamed ? 1u : 0u;
    return RT_OK;
}

extern "C" int rt_get_counters(rt_ctx *ctx, rt_counters *out)
{
    if (!ctx || !out) return fail(RT_ERR_INVALID, "rt_get_counters: null argument");
    if (ctx->streamed) return fail(RT_ERR_INVALID, "rt_get_counters: the streamed kernel books no counters (rt_get_streamed)");
    if (!ctx->counted) return fail(RT_ERR_INVALID, "rt_get_counters: the last render was not done with RT_FLAG_COUNT");
    unsigned long long h[8];
    if (int rc = read_synced(ctx, h, ctx->d_counters, sizeof(h))) return rc;
    out->primary_rays = h[0];
    out->shadow_rays = h[1];
    out->reflect_rays = h[2];
    out->tests = h[3];
    out->hits = h[4];
    out->solves = h[5];
    out->tests_executed = h[6];
    out->cull_evals = h[7];
    return RT_OK;
}

extern "C" int rt_get_counters_detail(rt_ctx *ctx, rt_counters_detail *out)
{
    if (!ctx || !out) return fail(RT_ERR_INVALID, "rt_get_counters_detail: null argument");
    if (ctx->streamed) return fail(RT_ERR_INVALID, "rt_get_counters_detail: the streamed kernel books no counters (rt_get_streamed)");
    if (!ctx->counted) return fail(RT_ERR_INVALID, "rt_get_counters_detail: the last render was not done with RT_FLAG_COUNT");
    if (ctx->cfg.flags & RT_FLAG_SIMPLE) return fail(RT_ERR_INVALID, "rt_get_counters_detail: the simple kernel does not split its counters");
    unsigned long long h[21];
    if (int rc = read_synced(ctx, h, ctx->d_counters + 32, sizeof(h))) return rc;
    for (int i = 0; i < 4; i++) out->tests_executed[i] = h[i];
    for (int i = 0; i < 3; i++) out->solves[i] = h[4 + i];
    for (int i = 0; i < 5; i++) out->cull_evals[i] = h[7 + i];
    for (int i = 0; i < 4; i++) out->cubic_branch[i] = h[12 + i];
    out->shadow_rays_traced = h[16];
    out->hit_lights_shaded = h[17];
    out->primary_rays_formed = h[18];
    out->cubic_points = h[19];
    out->cubic_refused = h[20];
    return RT_OK;
}

extern "C" int rt_debug_counters(rt_ctx *ctx, uint64_t out[32])
{
    if (!ctx || !out) return fail(RT_ERR_INVALID, "rt_debug_counters: null argument");
    if (int rc = read_synced(ctx, out, ctx->d_counters, sizeof(uint64_t) * 32)) return rc;
    if (ctx->d_stamps) { // diagnostic build: sum the per-wave stamp rows into words 8..19
        std::vector<uint64_t> rows(ctx->n_stamp_rows * 16);
        RT_HIP(hipMemcpy(rows.data(), ctx->d_stamps, rows.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < 12; i++) out[8 + i] = 0;
        for (size_t r = 0; r < ctx->n_stamp_rows; r++)
            for (int i = 0; i < 12; i++) out[8 + i] += rows[r * 16 + i];
    }
    return RT_OK;
}

extern "C" int rt_debug_stamp_rows(rt_ctx *ctx, uint64_t *out, size_t max_rows, size_t *n_rows)
{
    if (!ctx || !n_rows) return fail(RT_ERR_INVALID, "rt_debug_stamp_rows: null argument");
    *n_rows = ctx->d_stamps ? ctx->n_stamp_rows : 0;
    if (!out || !ctx->d_stamps) return RT_OK;
    const size_t n = max_rows < ctx->n_stamp_rows ? max_rows : ctx->n_stamp_rows;
    return read_synced(ctx, out, ctx->d_stamps, n * 16 * sizeof(uint64_t));
}

// The box helper of the render kernel (rt_wave_box.hpp) alone: one wave per entry.  Staged in buffers of the call's own, on the stream of
// the context's last call, and waited for there, like read_behind_last_call.
extern "C" int rt_debug_wave_box(rt_ctx *ctx, const double *pts, const uint64_t *use_masks, uint32_t n_waves, float *out)
{
    if (!ctx || !pts || !use_masks || !out) return fail(RT_ERR_INVALID, "rt_debug_wave_box: null argument");
    if (n_waves == 0) return fail(RT_ERR_INVALID, "rt_debug_wave_box: n_waves is 0");
    if (n_waves > 65536u) return fail(RT_ERR_INVALID, "rt_debug_wave_box: n_waves %u exceeds 65536", n_waves);
    if (int rc = use_device(ctx)) return rc;
    hipStream_t stream = ctx->last_stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream) RT_HIP(hipStreamIsCapturing(stream, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(RT_ERR_INVALID, "rt_debug_wave_box: the context's stream is capturing; end the capture first");
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "lane masks");
    const size_t pts_bytes = sizeof(double) * 192u * (size_t) n_waves, mask_bytes = sizeof(uint64_t) * (size_t) n_waves, out_bytes = sizeof(float) * 6u * (size_t) n_waves;
    DevMem<double> d_pts;
    DevMem<unsigned long long> d_masks;
    DevMem<float> d_out;
    RT_HIP(d_pts.alloc(pts_bytes));
    RT_HIP(d_masks.alloc(mask_bytes));
    RT_HIP(d_out.alloc(out_bytes));
    RT_HIP(hipMemcpyAsync(d_pts, pts, pts_bytes, hipMemcpyHostToDevice, stream));
    RT_HIP(hipMemcpyAsync(d_masks, use_masks, mask_bytes, hipMemcpyHostToDevice, stream));
    const hipError_t e = rt_launch_wave_box(d_pts, d_masks, n_waves, d_out, stream);
    if (e != hipSuccess) {
        (void) hipStreamSynchronize(stream); // (the copies read the caller's arrays and write buffers this call frees)
        return fail(RT_ERR_DEVICE, "rt_debug_wave_box: kernel launch failed: %s", hipGetErrorString(e));
    }
    RT_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    return RT_OK;
}

extern "C" int rt_destroy(rt_ctx *ctx)
{
    if (!ctx) return RT_OK;
    (void) hipSetDevice(ctx->device); // (the members release what the context holds there)
    delete ctx;
    return RT_OK;
}
