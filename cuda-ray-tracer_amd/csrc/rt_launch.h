// rt_launch.h -- every launcher the kernel files export to the host (rt_capi.cpp), declared once.  The launchers have C linkage, which
// carries no types: this header is what both sides see, so a definition that disagrees with the call does not compile.  Included by
// rt_capi.cpp and by every .hip file that defines a launcher.
#ifndef RT_LAUNCH_H
#define RT_LAUNCH_H

#include <hip/hip_runtime.h>

#include "rt_scene_dev.h"
#include "rt_set_scene.h"

// name_<variant>: the kernel files that are compiled once per floating-point contraction mode (-DRT_VARIANT=strict|fast) define RT_SYM(name)
#define RT_CAT2(a, b) a##_##b
#define RT_CAT(a, b) RT_CAT2(a, b)
#ifdef RT_VARIANT
#define RT_SYM(name) RT_CAT(name, RT_VARIANT)
#endif
#define RT_PER_VARIANT(ret, name, ...)                \
    extern "C" ret RT_CAT(name, strict)(__VA_ARGS__); \
    extern "C" ret RT_CAT(name, fast)(__VA_ARGS__);

// rt_kernels.hip: the simple kernel, and the frame transport (the host calls the _strict ones: they do no arithmetic a contraction changes)
RT_PER_VARIANT(hipError_t, rt_launch_trace, const FrameArgs *fa, const DevObject *gobj, const DevLight *glight, void *fb, unsigned long long *counters, int rgba8,
               int count, hipStream_t stream)
RT_PER_VARIANT(hipError_t, rt_launch_assemble, const void *gathered, void *full, uint32_t width, uint32_t height, uint32_t world, uint32_t band_rows,
               uint32_t max_local_rows, int rgba8, hipStream_t stream)
RT_PER_VARIANT(hipError_t, rt_launch_pack_sparse, const void *fb, void *msg, uint32_t width, uint32_t local_rows, const uint32_t *bg, uint32_t cap, int rgba8,
               hipStream_t stream)
RT_PER_VARIANT(hipError_t, rt_launch_assemble_sparse, const void *gathered, void *full, uint32_t width, uint32_t height, uint32_t world, uint32_t band_rows,
               const uint32_t *bg, uint32_t cap, void *stamps, uint32_t max_tiles, uint32_t tag, int rgba8, hipStream_t stream)
// rt_wavefront.hip: the product kernel
RT_PER_VARIANT(size_t, rt_wavefront_lds_bytes, uint32_t stage_bytes, uint32_t n_lights, int has_mirror, uint32_t n_cull_spheres, int lean, uint32_t n_cub)
RT_PER_VARIANT(hipError_t, rt_launch_wavefront, const FrameArgs *fa, const DevObject *gobj, const DevLight *glight, void *fb, unsigned long long *counters, int count,
               const double *camx, const double *camy, hipStream_t stream)
// rt_adaptive.hip: the ray-list kernel of adaptive supersampling and the classifiers (the host calls classify*_strict)
RT_PER_VARIANT(hipError_t, rt_launch_ray_list, const FrameArgs *fa, const DevObject *gobj, const DevLight *glight, const double *camx, const double *camy,
               const uint32_t *list, const uint32_t *count_ptr, uint32_t n_items, uint32_t k, uint32_t grid, void *out, int rgba8, int count,
               unsigned long long *counters, hipStream_t stream)
RT_PER_VARIANT(hipError_t, rt_launch_classify, const void *p, const void *halo, uint32_t width, uint32_t height, uint32_t local_rows, uint32_t band_rows,
               uint32_t world, uint32_t rank, float tau, void *out, int rgba8, uint32_t *list, uint32_t *count, hipStream_t stream)
RT_PER_VARIANT(hipError_t, rt_launch_classify_geometry, const void *p, const void *halo, const int32_t *obj, const float *nrm, const void *ghalo, uint32_t width,
               uint32_t height, uint32_t local_rows, uint32_t band_rows, uint32_t world, uint32_t rank, float tau, float min_cos, void *out, int rgba8,
               uint32_t *list, uint32_t *count, hipStream_t stream)
// The chunk bounds of a culling context, as the culled launchers take them: [n_chunks] UsEntry for the n_chunks = ceil(n_us / 64) chunks of the blob's
// (ordered) unit-sphere table, and the 8 work words the launch adds to (or NULL: nothing is counted)
struct ChunkTables {
    const void *bounds;
    uint32_t n_chunks;
    unsigned long long *stats;
};
// The seven queries.  Each has one signature for its three launchers -- the tables staged in LDS (rt_gbuffer.hip, rt_rays.hip, rt_shade_rays.hip,
// rt_paths.hip), streamed through a slice (rt_stream_queries.hip, RT_FLAG_STREAM_QUERIES) and streamed with chunks culled (rt_stream_cull_pixels.hip,
// RT_FLAG_STREAM_CULL_PIXELS; rt_stream_cull_rays.hip, RT_FLAG_STREAM_CULL_RAYS) --, so an entry point calls whichever the context decided on
// (struct QueryLaunchers below).  The staged and the streamed launchers ignore `chunks`.
// primary-hit G-buffer and picking (the two together: the G pass of an RT_FLAG_SSAA_GEOMETRY frame)
#define RT_GBUFFER_ARGS                                                                                                                              \
    const FrameArgs *fa, const void *scene, const double *camx, const double *camy, int32_t *out_object, double *out_t, float *out_normal, const ChunkTables *chunks, \
        hipStream_t stream
#define RT_PICK_ARGS \
    const FrameArgs *fa, const void *scene, const double *camx, const double *camy, const uint32_t *xy, uint32_t n, void *out, const ChunkTables *chunks, hipStream_t stream
// the object extents: the same rays reduced per object instead of stored (rect = x0, y0, x1, y1 inclusive, validated by the caller)
#define RT_OBJECT_EXTENTS_ARGS                                                                                                                        \
    const FrameArgs *fa, const void *scene, const double *camx, const double *camy, const uint32_t *rect, void *out, uint32_t max_grid, const ChunkTables *chunks, \
        hipStream_t stream
// caller-supplied rays: closest hit, occlusion, colour
#define RT_TRACE_RAYS_ARGS const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, void *out, uint32_t max_grid, const ChunkTables *chunks, hipStream_t stream
#define RT_OCCLUDED_RAYS_ARGS \
    const FrameArgs *fa, const void *scene, const void *rays, const double *t_max, uint32_t n, int32_t *out, uint32_t max_grid, const ChunkTables *chunks, hipStream_t stream
#define RT_SHADE_RAYS_ARGS                                                                                                                            \
    const FrameArgs *fa, const void *scene, const void *lights, const void *rays, uint32_t n, float *rgba, void *hits, uint32_t max_grid, const ChunkTables *chunks, \
        hipStream_t stream
// the hits along a ray's mirror bounces
#define RT_TRACE_PATHS_ARGS                                                                                                                           \
    const FrameArgs *fa, const void *scene, const void *rays, uint32_t n, uint32_t max_segments, void *segments, void *last, void *ends, uint32_t max_grid, \
        const ChunkTables *chunks, hipStream_t stream
// rt_gbuffer.hip (and what sizes its LDS)
RT_PER_VARIANT(size_t, rt_gbuffer_lds_bytes, const FrameArgs *fa)
RT_PER_VARIANT(int, rt_extents_lds_accumulators, size_t table_bytes, uint32_t n_obj)
RT_PER_VARIANT(size_t, rt_extents_lds_bytes, const FrameArgs *fa)
RT_PER_VARIANT(hipError_t, rt_launch_gbuffer, RT_GBUFFER_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_pick, RT_PICK_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_object_extents, RT_OBJECT_EXTENTS_ARGS)
// rt_rays.hip, rt_shade_rays.hip, rt_paths.hip
RT_PER_VARIANT(size_t, rt_rays_lds_bytes, const FrameArgs *fa)
RT_PER_VARIANT(hipError_t, rt_launch_trace_rays, RT_TRACE_RAYS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_occluded_rays, RT_OCCLUDED_RAYS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_shade_rays, RT_SHADE_RAYS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_trace_paths, RT_TRACE_PATHS_ARGS)
// rt_stream_queries.hip
RT_PER_VARIANT(hipError_t, rt_launch_stream_gbuffer, RT_GBUFFER_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_stream_pick, RT_PICK_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_stream_object_extents, RT_OBJECT_EXTENTS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_stream_trace_rays, RT_TRACE_RAYS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_stream_occluded_rays, RT_OCCLUDED_RAYS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_stream_shade_rays, RT_SHADE_RAYS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_stream_trace_paths, RT_TRACE_PATHS_ARGS)
// rt_stream_cull_pixels.hip (the chunks culled by the block's cone), rt_stream_cull_rays.hip (per caller-supplied ray): the work words are the family's
RT_PER_VARIANT(hipError_t, rt_launch_pixel_cull_gbuffer, RT_GBUFFER_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_pixel_cull_pick, RT_PICK_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_pixel_cull_object_extents, RT_OBJECT_EXTENTS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_stream_cull_trace_rays, RT_TRACE_RAYS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_stream_cull_occluded_rays, RT_OCCLUDED_RAYS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_stream_cull_shade_rays, RT_SHADE_RAYS_ARGS)
RT_PER_VARIANT(hipError_t, rt_launch_stream_cull_trace_paths, RT_TRACE_PATHS_ARGS)
// rt_paths.hip: the context's own primary rays as explicit rays (rect = x0, y0, x1, y1 inclusive, or a pixel list)
RT_PER_VARIANT(hipError_t, rt_launch_primary_rays, const FrameArgs *fa, const double *camx, const double *camy, const uint32_t *rect, const uint32_t *xy, uint32_t n_list,
               void *out, uint32_t max_grid, hipStream_t stream)
// rt_stream.hip: the streamed frame kernel (scenes of any size)
RT_PER_VARIANT(hipError_t, rt_launch_stream, const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy, void *fb,
               hipStream_t stream)
// rt_stream_adaptive.hip: the streamed twin of rt_launch_ray_list (RT_FLAG_STREAM_ADAPTIVE): its arguments without the counters, scene = the blob
RT_PER_VARIANT(hipError_t, rt_launch_stream_ray_list, const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy,
               const uint32_t *list, const uint32_t *count_ptr, uint32_t n_items, uint32_t k, uint32_t grid, void *out, int rgba8, hipStream_t stream)
// rt_stream_cull.hip: the streamed frame kernel with whole chunks of the unit-sphere table culled (RT_FLAG_STREAM_CULL): rt_launch_stream's arguments and the chunks
RT_PER_VARIANT(hipError_t, rt_launch_stream_cull, const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy, void *fb,
               const ChunkTables *chunks, hipStream_t stream)
// rt_stream_cull_bounce.hip: rt_launch_stream_cull with the bounce rays culled per ray as well (RT_FLAG_STREAM_CULL_BOUNCE): its arguments and the bounce
// work words (8, NULL exactly where chunks->stats is NULL)
RT_PER_VARIANT(hipError_t, rt_launch_stream_cull_bounce, const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy, void *fb,
               const ChunkTables *chunks, unsigned long long *bounce_stats, hipStream_t stream)
// rt_stream_cull_adaptive.hip: rt_launch_stream_ray_list with the same chunks culled (rt_get_stream_cull_adaptive): its arguments and the chunks, with work
// words of its own
RT_PER_VARIANT(hipError_t, rt_launch_stream_cull_ray_list, const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy,
               const uint32_t *list, const uint32_t *count_ptr, uint32_t n_items, uint32_t k, uint32_t grid, void *out, int rgba8, const ChunkTables *chunks,
               hipStream_t stream)
// The group bounds of a context whose culled frame asks a second level first (RT_FLAG_STREAM_CULL_GROUPS): [n_groups] UsEntry for the n_groups =
// ceil(n_chunks / 64) groups of 64 consecutive chunk bounds, and the 8 group work words the launch adds to (NULL exactly where the chunks' words are)
struct GroupTables {
    const void *groups;
    uint32_t n_groups;
    unsigned long long *stats;
};
// rt_stream_cull_groups.hip: rt_launch_stream_cull_bounce's arguments and the groups; bounce != 0: the bounce rays are culled per ray as well, 0: they keep
// the full sweep of rt_launch_stream_cull (bounce_stats NULL)
RT_PER_VARIANT(hipError_t, rt_launch_stream_cull_groups, const FrameArgs *fa, const void *scene, const void *lights, const double *camx, const double *camy, void *fb,
               const ChunkTables *chunks, const GroupTables *groups, unsigned long long *bounce_stats, int bounce, hipStream_t stream)
// built once without FMA contraction and used by both variants: the supersampling resolve (rt_resolve.hip) and the scene update (rt_set_scene.hip)
extern "C" hipError_t rt_launch_resolve(const void *in, void *out, uint32_t width, uint32_t rows, uint32_t k, int rgba8, int nt, hipStream_t stream);
extern "C" hipError_t rt_launch_set_scene(const SetSceneArgs *args, hipStream_t stream);
// rt_reorder_scene.hip, built once likewise (the key and the bounds are the host's functions): the bytes of work space a table of n_us entries takes (0 for
// n_us == 0), and the re-sort of the blob's unit-sphere table t_us into the order of rtp::stream_cull_image with the chunk bounds rebuilt -- work holds
// at least rt_reorder_scene_work_size(n_us) bytes, n_us > 0, every entry's orig is below n_obj
extern "C" size_t rt_reorder_scene_work_size(uint32_t n_us);
extern "C" hipError_t rt_launch_reorder_scene(void *t_us, uint32_t n_us, uint32_t n_obj, void *bounds, void *work, uint32_t max_grid, hipStream_t stream);
// rt_group_bounds.hip, built once likewise (the bounds are the host's function): groups[G] = rtp::pack_chunk_bound over chunk bounds 64 G .., G below
// ceil(n_chunks / 64), from the chunk bounds as the stream holds them behind either update's launcher
extern "C" hipError_t rt_launch_group_bounds(const void *bounds, uint32_t n_chunks, void *groups, hipStream_t stream);

// how a query reads the class tables: staged in LDS, streamed through a slice, or streamed with whole chunks culled
enum TablePath { PATH_STAGED, PATH_STREAMED, PATH_CULLED };
// the seven query launchers of one path (the types are the same on every path)
struct QueryLaunchers {
    decltype(&rt_launch_gbuffer_strict) gbuffer;
    decltype(&rt_launch_pick_strict) pick;
    decltype(&rt_launch_object_extents_strict) object_extents;
    decltype(&rt_launch_trace_rays_strict) trace_rays;
    decltype(&rt_launch_occluded_rays_strict) occluded_rays;
    decltype(&rt_launch_shade_rays_strict) shade_rays;
    decltype(&rt_launch_trace_paths_strict) trace_paths;
};
// the launchers a context calls per variant; rt_create picks one of the two instances (rt_capi.cpp) from RT_FLAG_FAST
struct Kernels {
    // rt_render: the simple, the product, the streamed kernel, and the streamed one culling (rt_get_stream_cull, rt_get_stream_cull_bounce)
    decltype(&rt_launch_trace_strict) trace;
    decltype(&rt_launch_wavefront_strict) wavefront;
    decltype(&rt_launch_stream_strict) stream;
    decltype(&rt_launch_stream_cull_strict) stream_cull;
    decltype(&rt_launch_stream_cull_bounce_strict) stream_cull_bounce;
    // the halo and refine passes of an adaptive frame: staged, streamed (rt_get_streamed_adaptive), and streamed and culling (rt_get_stream_cull_adaptive)
    decltype(&rt_launch_ray_list_strict) ray_list;
    decltype(&rt_launch_stream_ray_list_strict) stream_ray_list;
    decltype(&rt_launch_stream_cull_ray_list_strict) stream_cull_ray_list;
    decltype(&rt_launch_primary_rays_strict) primary_rays;
    QueryLaunchers query[3]; // by TablePath
};

// the launchers of a groups context per variant, in a record of their own (struct Kernels is the contexts' without the flag); rt_create picks one of the two
// instances (rt_capi.cpp) from RT_FLAG_FAST
struct GroupLaunchers {
    decltype(&rt_launch_stream_cull_groups_strict) frame;
};

// rt_planes.hip, built once (no floating-point arithmetic in it): the reassembly of a gathered plane of 4-, 8- or 16-byte elements
// (slot_stride in elements) and the merge of [n_parts][n_obj] object-extent records
extern "C" hipError_t rt_launch_assemble_planes(const void *gathered, size_t slot_stride, void *full, uint32_t width, uint32_t height, uint32_t world, uint32_t band_rows,
                                                uint32_t elem_bytes, hipStream_t stream);
extern "C" hipError_t rt_launch_merge_extents(const void *parts, uint32_t n_parts, uint32_t n_obj, void *out, hipStream_t stream);
// rt_wave_box.hip, built once: the box helper of rt_wavefront.hip (rt_wave_box.hpp) alone, one wave per entry (rt_debug_wave_box); pts = [n_waves][64][3],
// use_masks = [n_waves], out = [n_waves][6]
extern "C" hipError_t rt_launch_wave_box(const double *pts, const unsigned long long *use_masks, uint32_t n_waves, float *out, hipStream_t stream);
// rt_sort_rays.hip, built once (the key is the order's definition, not a variant's): the bytes of work space n rays take (0 for n == 0); the
// sort -- sorted and keys may be NULL, work holds at least rt_sort_rays_work_size(n) bytes, n > 0 --; planes x n records of elem_bytes (a
// multiple of 4) gathered (dst[i] = src[perm[i]]) or scattered (dst[perm[i]] = src[i])
extern "C" size_t rt_sort_rays_work_size(uint32_t n);
extern "C" hipError_t rt_launch_sort_rays(const void *rays, uint32_t n, void *sorted, uint32_t *perm, uint32_t *keys, void *work, uint32_t max_grid, hipStream_t stream);
extern "C" hipError_t rt_launch_permute(const uint32_t *perm, uint32_t n, const void *src, void *dst, uint32_t elem_bytes, uint32_t planes, int scatter, uint32_t max_grid,
                                        hipStream_t stream);

#endif
