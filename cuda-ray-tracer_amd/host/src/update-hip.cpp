// update-hip.cpp -- the MI355X back end behind the reference's update.h contract.
//
// Defines the three symbols a render back end must provide (reference include/update.h:6-8) by
// adapting them onto the C ABI of libmi355rt.so (include/mi355rt.h).  It takes the place of
// src/update-cuda.cu in the reference's link line (src/CMakeLists.txt:22-23); INTEGRATION.md shows the
// build change.  Like the reference back ends it keeps its state in file scope: the host calls
// init_update once, update once per frame and cleanup_update once (src/ray-tracer.cpp:215,226,245).
//
// Errors: the reference's CUDA back end prints the failure and exits (include/helper_cuda_opengl.h:13-24);
// this one does the same through die().
#include "update.h"

#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mi355rt.h"

// Environment (read by init_update; the reference's back ends take their configuration at build time):
//   MI355RT_DEVICES=0,1,...   render on these GPUs (rows band-cyclic, RCCL gather to the first: libmi355rt_multi.so,
//                             loaded on demand so that a one-GPU host never needs librccl); default: the current device
//   MI355RT_PARTS=n           contexts per device in that mode (overlap of transfer and rendering), default 2
//   MI355RT_BAND_ROWS=n       rows per band in that mode, default 16
//   MI355RT_MULTI_SELF=1      one device in MI355RT_DEVICES: send its rows to itself through RCCL (RT_MULTI_SELF_EXCHANGE)
//   MI355RT_MULTI_BANDWISE=1  rows travel band by band straight into their place in the frame (RT_MULTI_BANDWISE)
//   MI355RT_MULTI_SPARSE=1    only the 16x16 tiles that are not pure background travel (RT_MULTI_SPARSE; update() then waits on the host
//                             for every context's message header); not together with MI355RT_MULTI_BANDWISE
//                             (the MI355RT_MULTI_* switches are on when the variable is set, whatever its value)
//   MI355RT_FORMAT=rgba8      framebuffer = iround(c*255) RGBA8, the format the reference's CUDA back end writes to its display
//                             surface (src/update-cuda.cu:149-156); default rgba32f, the CPU back end's floats (src/update-cpu.cpp:128-131)
//   MI355RT_SSAA=2|4          supersampling, k x k rays per pixel box-filtered into the frame (RT_FLAG_SSAA2 / RT_FLAG_SSAA4, include/mi355rt.h),
//                             one GPU or several; default: one ray per pixel
//   MI355RT_SSAA_ADAPTIVE=<tau>  with MI355RT_SSAA: supersample only the pixels whose 3x3 neighbourhood differs by more than tau in some
//                             channel (RT_FLAG_SSAA_ADAPTIVE, rt_set_ssaa_threshold); empty: the default 1/32; tau < 0: every pixel
//   MI355RT_SSAA_GEOMETRY=<min_cos>  with MI355RT_SSAA_ADAPTIVE: also supersample the pixels next to one whose primary ray hits another
//                             object (RT_FLAG_SSAA_GEOMETRY, rt_set_ssaa_geometry); empty: object boundaries only; a number: also where the
//                             normals of one object make a cosine below it
//   MI355RT_STREAM=1          render with the streamed frame kernel whatever the scene's size (RT_FLAG_STREAM; same frame).  A scene too large
//                             for a workgroup's LDS takes that kernel without being asked; not together with MI355RT_SSAA_ADAPTIVE
//   MI355RT_STREAM_QUERIES=1  picking, extents and the ray-query hooks take their streamed kernels where the scene is too large for a
//                             workgroup's LDS (RT_FLAG_STREAM_QUERIES; same answers) instead of refusing it
//   MI355RT_STREAM_ADAPTIVE=1 adaptive supersampling (MI355RT_SSAA_ADAPTIVE) takes its streamed passes where the scene is too large for
//                             a workgroup's LDS (RT_FLAG_STREAM_ADAPTIVE; same frame) instead of refusing it; needs MI355RT_SSAA_ADAPTIVE
//   MI355RT_STREAM_CULL=1     a streamed context keeps its unit spheres in a spatial order and culls them by 64-entry chunk
//                             (RT_FLAG_STREAM_CULL; same frame); nothing changes where the context is not streamed
//   MI355RT_STREAM_CULL_BOUNCE=1  ... and culls the chunks of its bounce rays per ray (RT_FLAG_STREAM_CULL_BOUNCE; same frame); nothing
//                             changes without MI355RT_STREAM_CULL, without mirrors or below 65 unit spheres
//   MI355RT_STREAM_CULL_RAYS=1  ... and the ray-query hooks (trace, shade, pick path) cull the chunks per ray (RT_FLAG_STREAM_CULL_RAYS;
//                             same answers); nothing changes without MI355RT_STREAM_CULL and MI355RT_STREAM_QUERIES or below 65 unit spheres
//   MI355RT_STREAM_CULL_PIXELS=1  ... and the pixel hooks (pick, extents) cull the chunks by the block's cone (RT_FLAG_STREAM_CULL_PIXELS;
//                             same answers); nothing changes without MI355RT_STREAM_CULL and MI355RT_STREAM_QUERIES or below 65 unit spheres
//   MI355RT_STREAM_CULL_REORDER=1  ... and mi355rt_update_scene puts the unit spheres back into that spatial order behind every applied update
//                             (RT_FLAG_STREAM_CULL_REORDER, rt_reorder_scene; same frame); nothing changes without MI355RT_STREAM_CULL
//   MI355RT_STREAM_CULL_GROUPS=1  ... and the culled frame asks a second level of bounds first, one per 64 chunk bounds
//                             (RT_FLAG_STREAM_CULL_GROUPS; same frame); nothing changes without MI355RT_STREAM_CULL or below 4 097 unit spheres
namespace {

rt_ctx *g_ctx = nullptr;
rt_multi *g_multi = nullptr;
bool g_reorder = false; // MI355RT_STREAM_CULL_REORDER=1: mi355rt_update_scene reorders behind every applied update
void *g_multi_lib = nullptr;
struct MultiApi {
    int (*create)(rt_multi **, const rt_scene_desc *, const int *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) = nullptr;
    int (*render)(rt_multi *, const double *, void *, float *) = nullptr;
    int (*download)(rt_multi *, void *, size_t) = nullptr;
    int (*destroy)(rt_multi *) = nullptr;
    int (*set_threshold)(rt_multi *, float) = nullptr;
    int (*set_geometry)(rt_multi *, float) = nullptr;
    rt_ctx *(*query_ctx)(rt_multi *) = nullptr;
    void *(*stream)(rt_multi *) = nullptr;
    int (*set_scene)(rt_multi *, const rt_scene_update *) = nullptr;
    int (*scene_status)(rt_multi *, uint64_t *, uint64_t *, uint32_t *, uint32_t *) = nullptr;
    int (*reorder_scene)(rt_multi *) = nullptr;
} g_mapi;
unsigned int g_texture = 0;
unsigned int g_width = 0, g_height = 0;
uint32_t g_format = RT_FMT_RGBA32F;
// Optional presentation hooks: an interactive host that wants the frame in its GL texture installs a function that
// receives the rows (bottom row first) -- RGBA32F floats (what the CPU back end hands to glTexImage2D, src/update-cpu.cpp:136-137)
// or, with MI355RT_FORMAT=rgba8, RGBA8 bytes.  Headless use leaves them null and reads the device buffer.
void (*g_present)(unsigned int texture, unsigned int width, unsigned int height, const float *rgba) = nullptr;
void (*g_present8)(unsigned int texture, unsigned int width, unsigned int height, const unsigned char *rgba) = nullptr;
std::vector<unsigned char> g_staging;
double g_last_cam[16];     // the camera of the last update() call: what mi355rt_update_pick picks with
bool g_have_cam = false;

[[noreturn]] void die(const char *what)
{
    std::fprintf(stderr, "mi355rt: %s: %s\n", what, rt_last_error());
    std::exit(EXIT_FAILURE);
}

[[noreturn]] void die_text(const char *what, const char *why)
{
    std::fprintf(stderr, "mi355rt: %s: %s\n", what, why);
    std::exit(EXIT_FAILURE);
}

std::vector<int> device_list()
{
    std::vector<int> out;
    const char *env = std::getenv("MI355RT_DEVICES");
    if (!env || !*env) return out;
    const char *p = env;
    while (*p) {
        char *end = nullptr;
        long v = std::strtol(p, &end, 10);
        if (end == p || v < 0) die_text("MI355RT_DEVICES", "expected a comma-separated list of device ordinals");
        out.push_back((int) v);
        p = end;
        if (*p == ',') p++;
        else if (*p) die_text("MI355RT_DEVICES", "expected a comma-separated list of device ordinals");
    }
    return out;
}

uint32_t env_u32(const char *name, uint32_t dflt)
{
    const char *e = std::getenv(name);
    return (e && *e) ? (uint32_t) std::strtoul(e, nullptr, 10) : dflt;
}

void load_multi()
{
    if (g_multi_lib) return;
    // next to this library first (the build puts both in one directory), then the loader's search path
    Dl_info info{};
    std::string path = "libmi355rt_multi.so";
    if (dladdr((void *) &load_multi, &info) && info.dli_fname) {
        std::string here = info.dli_fname;
        const size_t slash = here.rfind('/');
        if (slash != std::string::npos) path = here.substr(0, slash + 1) + "libmi355rt_multi.so";
    }
    g_multi_lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!g_multi_lib) g_multi_lib = dlopen("libmi355rt_multi.so", RTLD_NOW | RTLD_LOCAL);
    if (!g_multi_lib) die_text("MI355RT_DEVICES needs libmi355rt_multi.so", dlerror());
    g_mapi.create = (decltype(g_mapi.create)) dlsym(g_multi_lib, "rt_create_multi");
    g_mapi.render = (decltype(g_mapi.render)) dlsym(g_multi_lib, "rt_render_multi");
    g_mapi.download = (decltype(g_mapi.download)) dlsym(g_multi_lib, "rt_multi_download");
    g_mapi.destroy = (decltype(g_mapi.destroy)) dlsym(g_multi_lib, "rt_multi_destroy");
    g_mapi.set_threshold = (decltype(g_mapi.set_threshold)) dlsym(g_multi_lib, "rt_multi_set_ssaa_threshold");
    g_mapi.set_geometry = (decltype(g_mapi.set_geometry)) dlsym(g_multi_lib, "rt_multi_set_ssaa_geometry");
    g_mapi.query_ctx = (decltype(g_mapi.query_ctx)) dlsym(g_multi_lib, "rt_multi_query_ctx");
    g_mapi.stream = (decltype(g_mapi.stream)) dlsym(g_multi_lib, "rt_multi_stream");
    g_mapi.set_scene = (decltype(g_mapi.set_scene)) dlsym(g_multi_lib, "rt_set_scene_multi");
    g_mapi.scene_status = (decltype(g_mapi.scene_status)) dlsym(g_multi_lib, "rt_multi_set_scene_status");
    g_mapi.reorder_scene = (decltype(g_mapi.reorder_scene)) dlsym(g_multi_lib, "rt_reorder_scene_multi");
    if (!g_mapi.create || !g_mapi.render || !g_mapi.download || !g_mapi.destroy || !g_mapi.set_threshold || !g_mapi.set_geometry || !g_mapi.query_ctx || !g_mapi.stream ||
        !g_mapi.set_scene || !g_mapi.scene_status || !g_mapi.reorder_scene)
        die_text("libmi355rt_multi.so", "missing entry points");
}

// the Scene's objects and lights as the ABI's flat arrays
struct FlatScene {
    std::vector<double> coefs, light_p;
    std::vector<float> refl, albedo, light_c;
    std::vector<uint8_t> kind;
    explicit FlatScene(const Scene &scene)
    {
        const size_t no = scene.objects.size(), nl = scene.lights.size();
        coefs.resize(no * RT_NCOEF);
        light_p.resize(nl * 3);
        refl.resize(no);
        albedo.resize(no * 3);
        light_c.resize(nl * 3);
        kind.resize(nl);
        for (size_t i = 0; i < no; i++) {
            const Object &o = scene.objects[i];
            const double *c = &o.surface.x3; // 20 packed doubles in SurfaceCoefs order (include/surface.h:12-14)
            for (int k = 0; k < RT_NCOEF; k++) coefs[i * RT_NCOEF + k] = c[k];
            refl[i] = o.reflection_ratio;
            for (int k = 0; k < 3; k++) albedo[3 * i + k] = o.color[k];
        }
        for (size_t i = 0; i < nl; i++) {
            const LightSource &l = scene.lights[i];
            kind[i] = l.is_spherical ? 1 : 0;
            for (int k = 0; k < 3; k++) {
                light_p[3 * i + k] = l.p[k];
                light_c[3 * i + k] = l.light_color[k];
            }
        }
    }
};
size_t g_n_objects = 0, g_n_lights = 0; // of the scene init_update() loaded: what mi355rt_update_scene may replace
std::vector<uint8_t> g_light_kind;

// The context the queries run on and its stream: the single context on the default stream, or with several devices the multi-GPU
// object's query context on its root stream (behind mi355rt_update_scene's update of the root).  NULL before init_update().
rt_ctx *query_ctx(void **stream)
{
    *stream = g_multi ? g_mapi.stream(g_multi) : nullptr;
    return g_multi ? g_mapi.query_ctx(g_multi) : g_ctx;
}

} // namespace

// Exported so a host can install / query without new headers.
extern "C" void mi355rt_set_presenter(void (*fn)(unsigned int, unsigned int, unsigned int, const float *)) { g_present = fn; }
extern "C" void mi355rt_set_presenter_rgba8(void (*fn)(unsigned int, unsigned int, unsigned int, const unsigned char *)) { g_present8 = fn; }
extern "C" rt_ctx *mi355rt_update_context(void) { return g_ctx; }
// Blocking copy of the last frame ([height][width] pixels of the configured format), whichever mode is active.
extern "C" int mi355rt_update_download(void *host_dst, size_t bytes)
{
    if (g_multi) return g_mapi.download(g_multi, host_dst, bytes);
    if (g_ctx) return rt_download(g_ctx, host_dst, bytes);
    return RT_ERR_INVALID;
}
extern "C" unsigned int mi355rt_update_format(void) { return g_format; }
// What lies under pixel (x, y) (row 0 = bottom) of the frame the last update() drew: rt_pick with that call's camera.  Single-context
// back end only: RT_ERR_INVALID with MI355RT_DEVICES naming several devices (tests/test_gbuffer_gpu.py pins that answer; there
// mi355rt_update_pick_path with max_segments = 1 returns the same record, and a caller of the C ABI has rt_multi_query_ctx), before the
// first update(), and for supersampling contexts.
extern "C" int mi355rt_update_pick(unsigned int x, unsigned int y, rt_hit *out)
{
    if (!g_ctx || !g_have_cam || !out) {
        rt_set_last_error(g_multi ? "mi355rt_update_pick: not available with several devices (MI355RT_DEVICES)"
                                  : (!out ? "mi355rt_update_pick: null argument" : "mi355rt_update_pick: no update() call yet"));
        return RT_ERR_INVALID;
    }
    const uint32_t xy[2] = {x, y};
    return rt_pick(g_ctx, g_last_cam, xy, 1, out, nullptr);
}

// Pick through mirrors: the path of pixel (x, y)'s primary ray along its mirror bounces (rt_pick_paths with the camera of the last
// update()): `segments` receives max_segments rt_hit records (NULL iff max_segments == 0; segments the path did not reach are miss
// records), *end what the pixel finally shows.  One device or several (the multi-GPU object's query context); RT_ERR_INVALID before the
// first update() and for supersampling contexts.
extern "C" int mi355rt_update_pick_path(unsigned int x, unsigned int y, rt_hit *segments, unsigned int max_segments, rt_path_end *end)
{
    void *stream = nullptr;
    rt_ctx *ctx = query_ctx(&stream);
    if (!ctx || !g_have_cam || !end) {
        rt_set_last_error(!end ? "mi355rt_update_pick_path: null argument" : "mi355rt_update_pick_path: no update() call yet");
        return RT_ERR_INVALID;
    }
    const uint32_t xy[2] = {x, y};
    return rt_pick_paths(ctx, g_last_cam, xy, 1, max_segments, segments, end, stream);
}

// Which objects the frame of the last update() shows, where and how far away: rt_object_extents_host with that call's camera, for the
// pixels of rect = x0, y0, x1, y1 (inclusive; NULL = the whole frame); n = the number of objects of the loaded scene, one record each.
// Single-context back end only: RT_ERR_INVALID with MI355RT_DEVICES naming several devices (a caller of the C ABI has
// rt_object_extents_multi), before the first update(), for another n and for supersampling contexts.
extern "C" int mi355rt_update_extents(const unsigned rect[4], rt_object_extent *out, unsigned n)
{
    if (!g_ctx || !g_have_cam || !out) {
        rt_set_last_error(g_multi ? "mi355rt_update_extents: not available with several devices (MI355RT_DEVICES)"
                                  : (!out ? "mi355rt_update_extents: null argument" : "mi355rt_update_extents: no update() call yet"));
        return RT_ERR_INVALID;
    }
    if (n != g_n_objects) {
        rt_set_last_error("mi355rt_update_extents: n must be the number of objects init_update() loaded");
        return RT_ERR_INVALID;
    }
    return rt_object_extents_host(g_ctx, g_last_cam, rect, out, nullptr);
}

// The closest hit of n caller-supplied rays against the scene init_update() loaded (rt_trace_rays_host; include/mi355rt.h, "Ray
// queries").  Valid after init_update(): unlike picking it needs no earlier update() call, a ray query uses no camera.  One device or
// several (the multi-GPU object's query context); RT_ERR_INVALID before init_update().
extern "C" int mi355rt_update_trace(const rt_ray *rays, unsigned int n, rt_hit *out)
{
    void *stream = nullptr;
    rt_ctx *ctx = query_ctx(&stream);
    if (!ctx) {
        rt_set_last_error("mi355rt_update_trace: no init_update() call yet");
        return RT_ERR_INVALID;
    }
    return rt_trace_rays_host(ctx, rays, n, out, stream);
}

// The reference's colour of n caller-supplied rays (rt_shade_rays_host; include/mi355rt.h, "Ray queries"): n x 4 float32, (r, g, b, 1).
// Valid after init_update() like mi355rt_update_trace, and refused where that is.
extern "C" int mi355rt_update_shade(const rt_ray *rays, unsigned int n, float *rgba_out)
{
    void *stream = nullptr;
    rt_ctx *ctx = query_ctx(&stream);
    if (!ctx) {
        rt_set_last_error("mi355rt_update_shade: no init_update() call yet");
        return RT_ERR_INVALID;
    }
    return rt_shade_rays_host(ctx, rays, n, rgba_out, stream);
}

// Move the objects and lights of the scene init_update() loaded: the same number of objects and lights, every light of its kind, the new
// coefficients, materials, light vectors and colours (rt_set_scene_host; include/mi355rt.h, "Scene updates").  Valid after init_update();
// the next update() draws the new scene.  RT_ERR_SCENE when the update would change the scene's layout (nothing is written then),
// RT_ERR_INVALID for other counts or kinds and before init_update().  With several devices (MI355RT_DEVICES) every context is updated
// (rt_set_scene_multi) and the call waits for all of them (rt_multi_set_scene_status).  Image size, background, field of view and
// max_reflections of `scene` are not looked at.
extern "C" int mi355rt_update_scene(const Scene &scene)
{
    if (!g_ctx && !g_multi) {
        rt_set_last_error("mi355rt_update_scene: no init_update() call yet");
        return RT_ERR_INVALID;
    }
    const FlatScene flat(scene);
    if (scene.objects.size() != g_n_objects || scene.lights.size() != g_n_lights || flat.kind != g_light_kind) {
        rt_set_last_error("mi355rt_update_scene: the number of objects and lights and every light's kind must stay what init_update() loaded");
        return RT_ERR_INVALID;
    }
    if (g_n_objects == 0 && g_n_lights == 0) return RT_OK;
    rt_scene_update u{};
    if (g_n_objects) {
        u.coefs = flat.coefs.data();
        u.reflection = flat.refl.data();
        u.albedo = flat.albedo.data();
    }
    if (g_n_lights) {
        u.light_p = flat.light_p.data();
        u.light_color = flat.light_c.data();
    }
    if (!g_multi) {
        if (int rc = rt_set_scene_host(g_ctx, &u, nullptr)) return rc;
        return g_reorder ? rt_reorder_scene(g_ctx, nullptr) : RT_OK;
    }
    uint64_t before = 0, after = 0;
    uint32_t reason = 0, index = 0;
    if (int rc = g_mapi.scene_status(g_multi, nullptr, &before, nullptr, nullptr)) return rc;
    if (int rc = g_mapi.set_scene(g_multi, &u)) return rc;
    if (int rc = g_mapi.scene_status(g_multi, nullptr, &after, &reason, &index)) return rc;
    if (after != before) {
        char text[160];
        std::snprintf(text, sizeof(text), "mi355rt_update_scene: update rejected by every context, nothing was written: reason %u at index %u: see RT_SCENE_REJECT_*", reason, index);
        rt_set_last_error(text);
        return RT_ERR_SCENE;
    }
    return g_reorder ? g_mapi.reorder_scene(g_multi) : RT_OK;
}

void init_update(unsigned int texture, const Scene &scene)
{
    if (g_ctx || g_multi) cleanup_update();
    g_texture = texture;
    g_width = scene.px_width;
    g_height = scene.px_height;
    g_format = RT_FMT_RGBA32F;
    g_have_cam = false;
    if (const char *f = std::getenv("MI355RT_FORMAT")) {
        if (!std::strcmp(f, "rgba8")) g_format = RT_FMT_RGBA8;
        else if (std::strcmp(f, "rgba32f") && *f) die_text("MI355RT_FORMAT", "expected rgba32f or rgba8");
    }
    uint32_t ssaa = 0;
    if (const char *f = std::getenv("MI355RT_SSAA")) {
        if (!std::strcmp(f, "2")) ssaa = RT_FLAG_SSAA2;
        else if (!std::strcmp(f, "4")) ssaa = RT_FLAG_SSAA4;
        else if (*f) die_text("MI355RT_SSAA", "expected 2 or 4");
    }
    // MI355RT_STREAM=1: the streamed frame kernel whatever the scene's size (scenes too large for LDS take it without being asked)
    uint32_t streamed = 0;
    if (const char *f = std::getenv("MI355RT_STREAM")) {
        if (!std::strcmp(f, "1")) streamed = RT_FLAG_STREAM;
        else if (std::strcmp(f, "0") && *f) die_text("MI355RT_STREAM", "expected 0 or 1");
    }
    // MI355RT_STREAM_QUERIES=1: the queries of a scene too large for LDS take their streamed kernels instead of refusing
    if (const char *f = std::getenv("MI355RT_STREAM_QUERIES")) {
        if (!std::strcmp(f, "1")) streamed |= RT_FLAG_STREAM_QUERIES;
        else if (std::strcmp(f, "0") && *f) die_text("MI355RT_STREAM_QUERIES", "expected 0 or 1");
    }
    // MI355RT_STREAM_ADAPTIVE=1: adaptive supersampling of a scene too large for LDS takes its streamed passes instead of refusing
    if (const char *f = std::getenv("MI355RT_STREAM_ADAPTIVE")) {
        if (!std::strcmp(f, "1")) streamed |= RT_FLAG_STREAM_ADAPTIVE;
        else if (std::strcmp(f, "0") && *f) die_text("MI355RT_STREAM_ADAPTIVE", "expected 0 or 1");
    }
    // MI355RT_STREAM_CULL=1: a streamed context culls whole chunks of its unit-sphere table
    if (const char *f = std::getenv("MI355RT_STREAM_CULL")) {
        if (!std::strcmp(f, "1")) streamed |= RT_FLAG_STREAM_CULL;
        else if (std::strcmp(f, "0") && *f) die_text("MI355RT_STREAM_CULL", "expected 0 or 1");
    }
    // MI355RT_STREAM_CULL_BOUNCE=1: ... and the chunks of its bounce rays, per ray
    if (const char *f = std::getenv("MI355RT_STREAM_CULL_BOUNCE")) {
        if (!std::strcmp(f, "1")) streamed |= RT_FLAG_STREAM_CULL_BOUNCE;
        else if (std::strcmp(f, "0") && *f) die_text("MI355RT_STREAM_CULL_BOUNCE", "expected 0 or 1");
    }
    // MI355RT_STREAM_CULL_RAYS=1: ... and the chunks of the ray-query hooks' rays, per ray
    if (const char *f = std::getenv("MI355RT_STREAM_CULL_RAYS")) {
        if (!std::strcmp(f, "1")) streamed |= RT_FLAG_STREAM_CULL_RAYS;
        else if (std::strcmp(f, "0") && *f) die_text("MI355RT_STREAM_CULL_RAYS", "expected 0 or 1");
    }
    // MI355RT_STREAM_CULL_PIXELS=1: ... and the chunks of the pixel hooks (pick, extents), by the block's cone
    if (const char *f = std::getenv("MI355RT_STREAM_CULL_PIXELS")) {
        if (!std::strcmp(f, "1")) streamed |= RT_FLAG_STREAM_CULL_PIXELS;
        else if (std::strcmp(f, "0") && *f) die_text("MI355RT_STREAM_CULL_PIXELS", "expected 0 or 1");
    }
    // MI355RT_STREAM_CULL_GROUPS=1: ... and the culled frame asks a second level of bounds first, one per 64 chunk bounds
    if (const char *f = std::getenv("MI355RT_STREAM_CULL_GROUPS")) {
        if (!std::strcmp(f, "1")) streamed |= RT_FLAG_STREAM_CULL_GROUPS;
        else if (std::strcmp(f, "0") && *f) die_text("MI355RT_STREAM_CULL_GROUPS", "expected 0 or 1");
    }
    // MI355RT_STREAM_CULL_REORDER=1: ... and mi355rt_update_scene re-sorts the unit spheres behind every applied update
    g_reorder = false;
    if (const char *f = std::getenv("MI355RT_STREAM_CULL_REORDER")) {
        if (!std::strcmp(f, "1")) streamed |= RT_FLAG_STREAM_CULL_REORDER, g_reorder = true;
        else if (std::strcmp(f, "0") && *f) die_text("MI355RT_STREAM_CULL_REORDER", "expected 0 or 1");
    }
    bool adaptive = false;
    float tau = 1.0f / 32.0f;
    if (const char *f = std::getenv("MI355RT_SSAA_ADAPTIVE")) {
        if (!ssaa) die_text("MI355RT_SSAA_ADAPTIVE", "needs MI355RT_SSAA=2 or 4");
        adaptive = true;
        if (*f) {
            char *end = nullptr;
            tau = std::strtof(f, &end);
            if (*end || std::isnan(tau)) die_text("MI355RT_SSAA_ADAPTIVE", "expected a threshold (a number, or empty for the default 1/32)");
        }
        ssaa |= RT_FLAG_SSAA_ADAPTIVE;
    }
    bool geometry = false, have_min_cos = false;
    float min_cos = 0.0f;
    if (const char *f = std::getenv("MI355RT_SSAA_GEOMETRY")) {
        if (!adaptive) die_text("MI355RT_SSAA_GEOMETRY", "needs MI355RT_SSAA_ADAPTIVE");
        geometry = true;
        if (*f) {
            char *end = nullptr;
            min_cos = std::strtof(f, &end);
            if (*end || std::isnan(min_cos)) die_text("MI355RT_SSAA_GEOMETRY", "expected a cosine (a number, or empty for object boundaries only)");
            have_min_cos = true;
        }
        ssaa |= RT_FLAG_SSAA_GEOMETRY;
    }

    // flatten the Scene into the ABI's descriptor (arrays are borrowed only for the call)
    const size_t no = scene.objects.size(), nl = scene.lights.size();
    const FlatScene flat(scene);
    const std::vector<double> &coefs = flat.coefs, &light_p = flat.light_p;
    const std::vector<float> &refl = flat.refl, &albedo = flat.albedo, &light_c = flat.light_c;
    const std::vector<uint8_t> &kind = flat.kind;
    g_n_objects = no;
    g_n_lights = nl;
    g_light_kind = kind;
    rt_scene_desc sd{};
    sd.width = scene.px_width;
    sd.height = scene.px_height;
    sd.vertical_fov = scene.vertical_fov;
    for (int k = 0; k < 3; k++) sd.bg_color[k] = scene.bg_color[k];
    sd.max_reflections = scene.max_reflections;
    sd.n_objects = (uint32_t) no;
    sd.n_lights = (uint32_t) nl;
    sd.coefs = coefs.data();
    sd.reflection = refl.data();
    sd.albedo = albedo.data();
    sd.light_is_spherical = kind.data();
    sd.light_p = light_p.data();
    sd.light_color = light_c.data();

    const std::vector<int> devs = device_list();
    if (devs.size() > 1 || (devs.size() == 1 && std::getenv("MI355RT_MULTI_SELF"))) {
        load_multi();
        if (std::getenv("MI355RT_MULTI_SPARSE") && std::getenv("MI355RT_MULTI_BANDWISE"))
            die_text("init_update", "MI355RT_MULTI_SPARSE and MI355RT_MULTI_BANDWISE exclude each other (tiles travel as sparse messages, or rows band by band): set one");
        const uint32_t flags = RT_FLAG_STRICT | ssaa | streamed | (std::getenv("MI355RT_MULTI_SELF") ? RT_MULTI_SELF_EXCHANGE : 0u) |
                               (std::getenv("MI355RT_MULTI_BANDWISE") ? RT_MULTI_BANDWISE : 0u) | // (rows band by band into their place in the frame: no reassembly pass)
                               (std::getenv("MI355RT_MULTI_SPARSE") ? RT_MULTI_SPARSE : 0u);     // (only tiles with content travel)
        if (g_mapi.create(&g_multi, &sd, devs.data(), (uint32_t) devs.size(), env_u32("MI355RT_BAND_ROWS", 16), env_u32("MI355RT_PARTS", 2), flags, g_format) != RT_OK)
            die("init_update (MI355RT_DEVICES)");
        if (adaptive && g_mapi.set_threshold(g_multi, tau) != RT_OK) die("init_update (MI355RT_SSAA_ADAPTIVE)");
        if (geometry && have_min_cos && g_mapi.set_geometry(g_multi, min_cos) != RT_OK) die("init_update (MI355RT_SSAA_GEOMETRY)");
        return;
    }
    rt_config cfg{};
    cfg.device = devs.empty() ? -1 : devs[0];
    cfg.world = 1;
    cfg.flags = RT_FLAG_STRICT | ssaa | streamed;
    cfg.format = g_format;
    if (rt_create(&g_ctx, &sd, &cfg) != RT_OK) die("init_update");
    if (adaptive && rt_set_ssaa_threshold(g_ctx, tau) != RT_OK) die("init_update (MI355RT_SSAA_ADAPTIVE)");
    if (geometry && have_min_cos && rt_set_ssaa_geometry(g_ctx, min_cos) != RT_OK) die("init_update (MI355RT_SSAA_GEOMETRY)");
}

float update(const glm::dmat4 &camera_matrix)
{
    if (!g_ctx && !g_multi) {
        std::fprintf(stderr, "mi355rt: update() called before init_update()\n");
        std::exit(EXIT_FAILURE);
    }
    double cam[16];
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) cam[c * 4 + r] = camera_matrix[c][r];
    std::memcpy(g_last_cam, cam, sizeof(cam));
    g_have_cam = true;
    float ms = 0.0f;
    if (g_multi) {
        if (g_mapi.render(g_multi, cam, nullptr, &ms) != RT_OK) die("update");
    } else if (rt_render(g_ctx, cam, nullptr, nullptr, &ms) != RT_OK) {
        die("update");
    }
    if ((g_format == RT_FMT_RGBA8 && g_present8) || (g_format == RT_FMT_RGBA32F && g_present)) {
        g_staging.resize((size_t) g_width * g_height * (g_format == RT_FMT_RGBA8 ? 4 : 16));
        if (mi355rt_update_download(g_staging.data(), g_staging.size()) != RT_OK) die("update (download)");
        if (g_format == RT_FMT_RGBA8) g_present8(g_texture, g_width, g_height, g_staging.data());
        else g_present(g_texture, g_width, g_height, reinterpret_cast<const float *>(g_staging.data()));
    }
    return ms; // device time of the frame, like src/update-cuda.cu:187-189 (several GPUs: transfers and reassembly included)
}

void cleanup_update()
{
    if (g_ctx) rt_destroy(g_ctx);
    g_ctx = nullptr;
    if (g_multi) g_mapi.destroy(g_multi);
    g_multi = nullptr;
    g_have_cam = false;
}
