/*
 * mi355rt.h -- C ABI of the MI355X-native per-pixel ray-tracing path (libmi355rt.so).
 *
 * This is the drop-in boundary underneath the reference's C++ back-end interface.  The reference
 * selects a back end at link time by defining three functions (include/update.h:6-8) on top of the
 * scene model (include/scene.h:8-36) filled by its YAML loader (src/scene.cpp:154-203).  Each entry
 * point below names the reference interface it replaces; cuda-ray-tracer_amd/host/src/update-hip.cpp
 * is the adapter that implements update.h on this ABI, INTEGRATION.md shows how a maintainer of
 * the reference links it.
 *
 * Conventions: plain pointers and sizes only, no C++/torch types; every function returns RT_OK (0) or a
 * negative rt_status and never throws; rt_last_error() gives the message of the calling thread's last
 * failure.  A context belongs to one thread at a time (the reference back ends keep their state in
 * file-scope globals, src/update-cpu.cpp:10-19; here it is an explicit object).
 */
#ifndef MI355RT_H
#define MI355RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 3
#define RT_ABI_DIAGNOSTIC 0x4000 /* set in rt_abi_version() of a library built with STAMPS / DEBUG_EXITS / SPILLS_OK / ...: for
                                    measurements only (it may spill registers to scratch, which the product never does) */

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = -1,   /* bad argument */
    RT_ERR_SCENE = -2,     /* scene description rejected (what SceneException reports in the reference) */
    RT_ERR_DEVICE = -3,    /* HIP runtime error */
    RT_ERR_NO_DEVICE = -4, /* no usable GPU: the product has no CPU fallback */
    RT_ERR_NOMEM = -5
} rt_status;

/* Number of doubles per surface: SurfaceCoefs, include/surface.h:10-15, same order
 * x3 y3 z3 x2y xy2 x2z xz2 y2z yz2 xyz x2 y2 z2 xy xz yz x y z c */
#define RT_NCOEF 20

/* Flat view of a Scene (include/scene.h:17-36).  Arrays are borrowed for the duration of the call
 * that receives the descriptor (the reference back ends copy the scene too, src/update-cpu.cpp:29-30). */
typedef struct rt_scene_desc {
    uint32_t width, height;        /* Scene::px_width / px_height */
    double vertical_fov;           /* Scene::vertical_fov, RADIANS */
    float bg_color[3];             /* Scene::bg_color */
    uint32_t max_reflections;      /* Scene::max_reflections */
    uint32_t n_objects;            /* Scene::objects.size() */
    uint32_t n_lights;             /* Scene::lights.size() */
    const double *coefs;           /* [n_objects][RT_NCOEF]   Object::surface */
    const float *reflection;       /* [n_objects]             Object::reflection_ratio */
    const float *albedo;           /* [n_objects][3]          Object::color */
    const uint8_t *light_is_spherical; /* [n_lights]          LightSource::is_spherical */
    const double *light_p;         /* [n_lights][3]           LightSource::p (direction already -normalised) */
    const float *light_color;      /* [n_lights][3]           LightSource::light_color (intensity folded in) */
} rt_scene_desc;

/* rt_config.flags */
#define RT_FLAG_STRICT 0u     /* default: FP64 geometry / FP32 colour with NO FMA contraction -- the arithmetic
                                 of src/update-cpu.cpp on x86-64; this is the parity mode */
#define RT_FLAG_FAST 1u       /* same algorithm with FMA contraction allowed.  For surfaces of degree <= 2 the result of
                                 every ray whose decisions are not near-ties is the exact one up to rounding: `object` and
                                 the blocked flag are those of exact arithmetic, t is within the first-order running-error
                                 bound B of the exact root, point is o + t d to 2u per term, the normal is the exact normal
                                 at point to half a float32 ulp, and a frame's pixel is the strict frame's to 1e-5 relative.
                                 A near-tie is a decision (|t2| or |t1| against EPS, the discriminant's sign, a root against
                                 EPS, MAX_T or t_max, two objects' roots against each other) closer to its threshold than
                                 2^20 times its bound; only such rays may differ ("The FAST build against exact
                                 arithmetic"; tests/test_fast_truth_gpu.py).  Degree 3, in this and in the strict build: the
                                 same, with t within B3 + 1e-8 |t| of the exact root the reference's rule selects -- B3 the
                                 first-order bound of the reference's own cubic solver, 1e-8 what cubic_guarded (csrc/rt_math.hpp)
                                 allows itself -- and two objects' roots a near-tie also within 1e-8 of their sizes */
#define RT_FLAG_COUNT 2u      /* also count rays / intersection tests on the device (slower; for accounting) */
#define RT_FLAG_SIMPLE 4u     /* use the simple one-thread-per-pixel kernel (rt_kernels.hip) instead of the
                                 workgroup wavefront kernel (rt_wavefront.hip); same results, kept for A/B runs */
#define RT_FLAG_NOCULL 8u     /* wavefront kernel: test every object for every shadow ray (no bounding-volume
                                 culling); same results, kept for A/B runs and as a cross-check */
#define RT_FLAG_STATIC_ORDER 16u /* wavefront kernel: start the tiles in index order every frame instead of starting
                                 the tiles that had hits in the previous frame first; same results, for A/B runs */

#define RT_FLAG_NOSCAN 32u    /* wavefront kernel: no scan workgroups (every tile's own workgroup decides whether the tile is
                                 empty and paints it); same results, for A/B runs */

#define RT_FLAG_PLAIN_ORDER 64u /* wavefront kernel: the tiles that had hits start in plain descending-cost order instead of the order that
                                  balances the CUs' loads (rt_wavefront.hip, ord_rank_of_slot); same results, for A/B runs */
#define RT_FLAG_NOSPLIT 128u   /* wavefront kernel: every tile is rendered by one workgroup (default: the costliest tiles of the previous frame
                               * by two, one per half tile) -- for A/B */

#define RT_FLAG_NOLEAN 256u    /* wavefront kernel: scenes of unit spheres without mirrors are rendered by the general instantiation (hit queue per
                               * tile) instead of the wave-per-block one; same results, for A/B runs and as a cross-check */

/* Supersampling: k x k rays per output pixel (k = 2 or 4; at most one of the two flags).  The context renders the unmodified scene at
 * (k*width) x (k*height) into an internal RGBA32F frame S with the usual kernels -- sample (X, Y) of S is exactly the reference's pixel
 * (X, Y) at that size (aspect and tan(fov/2) do not change) -- and a resolve kernel box-filters it: sub-pixel (i, j) of output pixel
 * (x, y) is S[k*y + j][k*x + i] (row 0 = bottom); per channel, in FP32 without FMA contraction, every sub-row is summed as a pairwise
 * tree over i (k = 2: s0 + s1; k = 4: (s0 + s1) + (s2 + s3)), the sub-row sums by the same tree over j, the result multiplied by 1/k^2
 * (exact), alpha 1.0f.  RGBA8 quantises the average as the render kernels do, (unsigned char)(int)(v * 255.0f + 0.5f), alpha 255.  A
 * pixel whose samples are all equal resolves to exactly that value (a pure background pixel stays bit-equal to the background).
 * The resolve is the same in every variant (RT_FLAG_FAST included); the flags combine with every other RT_FLAG_*.  rt_create refuses
 * (RT_ERR_INVALID) both flags together and k*width or k*height above 65536, before it looks for a device.
 * Everything the caller sees describes the OUTPUT frame: rt_local_rows, rt_max_local_rows, rt_row_map, rt_pixel_bytes, rt_device_fb,
 * rt_download, rt_assemble, rt_pack_sparse, rt_assemble_sparse[_incremental], rt_sparse_stamp_bytes; bands are band_rows output rows
 * (the internal frame uses k*band_rows internal rows per band, so output band b comes from internal band b and row ownership does
 * not change).  rt_render renders into the internal buffer (k^2 * width * local_rows * 16 bytes, allocated by rt_create) and resolves
 * into dev_fb or the context's own buffer, both kernels on `stream`; `ms` covers both, the ordering event is recorded behind the
 * resolve, and a frame can be captured into a graph as before (two kernels per frame).  rt_render_sparse renders, resolves into the
 * context's own buffer and packs it with rt_pack_sparse: the message holds the same tiles as rt_render + rt_pack_sparse.
 * RT_FLAG_COUNT counts the rays actually traced: primary_rays = k^2 * width * height. */
#define RT_FLAG_SSAA2 512u
#define RT_FLAG_SSAA4 1024u

/* Edge-adaptive supersampling: only valid together with exactly one of RT_FLAG_SSAA2 / RT_FLAG_SSAA4 (rt_create
 * refuses it alone with RT_ERR_INVALID before it looks for a device; the 65536-per-axis limit on k*width and k*height holds).  With
 * P = the plain frame (the reference's pixels at width x height, what a k = 1 context renders, in RGBA32F), S = the k x k sample frame
 * above and tau = the threshold (rt_set_ssaa_threshold, default 1/32):
 *   refine(x, y) = tau < 0, or some 8-neighbour n of (x, y) inside the image and some channel c of R, G, B gives
 *                  !(fabsf(P(x,y).c - P(n).c) <= tau)   (one float32 subtraction: NaN differences refine; band edges are not image edges)
 *   output(x, y) = the RT_FLAG_SSAAk resolve of S at (x, y) where refine(x, y), else P(x, y); alpha 1.0f; RGBA8 quantises either value
 *                  as the render kernels do.
 * So tau < 0 gives the RT_FLAG_SSAAk frame, tau = +inf the k = 1 frame (scenes without NaN colours), and a pure background pixel stays
 * the background.  rt_render runs, on `stream`: the plain pass (the usual render kernels, no k^2 frame is allocated), with world > 1 the
 * centre rays of the rows just outside each band (so every rank's rows equal the single-context frame's), a classify kernel (unrefined
 * pixels are written out, refined ones appended to a device list) and a kernel that traces the k^2 sample rays of the listed pixels.
 * Nothing is read back to the host, so frames can be captured into a graph.  `ms` covers all of it; RT_FLAG_COUNT counts every ray:
 * primary_rays = width * local_rows + halo rays + k^2 * refined (rt_get_counters_detail stays the wavefront kernel's). */
#define RT_FLAG_SSAA_ADAPTIVE 2048u

/* Geometric edges for the adaptive classifier: only valid together with RT_FLAG_SSAA_ADAPTIVE, and therefore with
 * exactly one of RT_FLAG_SSAA2 / RT_FLAG_SSAA4 (rt_create refuses it without RT_FLAG_SSAA_ADAPTIVE with RT_ERR_INVALID before it looks
 * for a device).  The colour term above cannot see a boundary between two surfaces that are lit alike (equal albedo under a head-on
 * light, an object of the background's colour, a scene without lights, the fold of a cubic over itself); this flag adds what the
 * primary ray hits.  In the notation above, with obj(x, y) and N(x, y) = the `object` entry and the first three `normal` floats of the
 * G-buffer definition below (the primary hit on the output frame's W x H grid; a miss gives -1 and three +0.0f) and c = the normal
 * threshold (rt_set_ssaa_geometry, default -inf):
 *   geo(x, y)    = some 8-neighbour n of (x, y) inside the image gives
 *                      obj(n) != obj(x, y)
 *                   or (obj(n) == obj(x, y) >= 0  and  !(dotf(N(x, y), N(n)) >= c))
 *   dotf(a, b)   = ((a.x * b.x) + (a.y * b.y)) + (a.z * b.z)   float32, every operation rounded separately, no FMA, identical in the
 *                  strict and RT_FLAG_FAST builds (as the resolve's sums are)
 *   refine(x, y) = refine of RT_FLAG_SSAA_ADAPTIVE (tau, colour)  or  geo(x, y)
 * The output rule is unchanged: the RT_FLAG_SSAAk resolve of S where refine(x, y), else P(x, y).  A NaN dot product refines, as a NaN
 * colour difference does; band edges are not image edges; only the primary hit counts (an edge seen in a mirror stays the colour
 * term's business).  tau < 0 still gives the full RT_FLAG_SSAAk frame, tau = +inf now means "geometric edges only", and a pure
 * background pixel whose eight neighbours are background stays the background pixel (so a sparse message holds the same tiles).
 * With c = -inf the normal term can only fire on a NaN normal (a hit exactly where a surface's gradient vanishes), and the library
 * does not form the normals at all then: object ids only, and such a pixel is not seen.  Any finite c <= -2 forms them and has
 * exactly the meaning the definition gives c = -inf.  No default crease angle is chosen: nobody has measured one.
 * In strict contexts obj and N are the G-buffer definition's values for surfaces of degree <= 2; in RT_FLAG_FAST contexts (and for
 * degree 3) they are bit for bit what rt_render_gbuffer / rt_pick report on a context without supersampling and otherwise equal flags
 * (the same kernel computes them, or -- RT_FLAG_STREAM_CULL_PIXELS -- its culling twin, bit-equal by that flag's rule).  rt_render
 * adds, on `stream`, that kernel for this rank's rows (and, world > 1, for the rows just outside each band) in front of the classify
 * kernel; still nothing is read back and frames can be captured into a graph.
 * rt_get_ssaa_refined and rt_render_sparse work as in every adaptive context.  RT_FLAG_COUNT does not book the rays of that pass (as
 * rt_render_gbuffer books none): primary_rays = width * local_rows + halo rays + k^2 * refined, with the new refined count.
 * Known limits: two sheets of ONE object at different depths whose normals agree are not told apart (there is no depth term), and a
 * mirror shows only itself (edges inside a reflection are not followed; rt_trace_paths reports what a mirror shows).  rt_render_gbuffer and rt_pick keep refusing every supersampling context. */
#define RT_FLAG_SSAA_GEOMETRY 4096u

/* Streamed frames: rt_render for scenes of any size.  The render kernels above keep the scene in a workgroup's LDS
 * (the wavefront kernel its class tables, the simple kernel the object records), which bounds a scene at roughly 1 700 spheres; the
 * streamed kernel (rt_stream.hip) leaves the tables in global memory and passes them through a wave-private LDS slice 64 entries at a
 * time.  A context is streamed -- rt_get_streamed says so -- when it was created with RT_FLAG_STREAM, or without RT_FLAG_SIMPLE for a
 * scene whose wavefront kernel would need more than 160 KiB of LDS, or with RT_FLAG_SIMPLE for more than 160 KiB of object records.
 * Definition: the frame of rt_render, by the arithmetic of rt_shade_rays on the rays of rt_primary_rays -- pixel (x, y) is the colour
 * rt_shade_rays gives the ray rt_primary_rays forms for (x, y), quantised for RGBA8 as the render kernels do.
 * Accuracy: in strict contexts bit-identical to the other render kernels (and the CPU reference) for surfaces of degree <= 2, in both
 * formats, and bit-identical to rt_shade_rays(rt_primary_rays) for every degree; degree-3 frames meet the bar of the other kernels'
 * degree-3 frames (1e-5 relative per channel, at most max(3, 0.2 % of the pixels) beyond it against the CPU reference).  RT_FLAG_FAST is
 * its own arithmetic (FMA contraction), held to 1e-5 relative like every RT_FLAG_FAST frame.  RT_FLAG_NOCULL switches the one piece of
 * work removal off (primary rays skip the spheres outside their 8 x 8 block's cone); same results.
 * A streamed context holds no frame-to-frame state: rt_render is one kernel (plus the resolve under RT_FLAG_SSAA2 / RT_FLAG_SSAA4),
 * captured and replayed freely.  Formats, ranks and bands, rt_pack_sparse and the assemble calls, rt_set_scene and the multi-GPU layer
 * work as on any context.
 * Refused: RT_FLAG_STREAM with RT_FLAG_SIMPLE, RT_FLAG_SSAA_ADAPTIVE (unless with RT_FLAG_STREAM_ADAPTIVE, below) or RT_FLAG_COUNT (RT_ERR_INVALID, before rt_create looks for a
 * device); RT_FLAG_COUNT for a scene that must be streamed, with or without RT_FLAG_SIMPLE (RT_ERR_SCENE: the streamed kernel books no
 * counters); rt_get_counters and
 * rt_get_counters_detail (RT_ERR_INVALID); rt_render_sparse (RT_ERR_INVALID, as with RT_FLAG_SIMPLE: rt_render + rt_pack_sparse give
 * the same message).
 * Out of scope: adaptive supersampling stages the scene in LDS and keeps its rt_create refusals unless the context was created with
 * RT_FLAG_STREAM_ADAPTIVE (below); the G-buffer, picking, object
 * extents, the ray queries and the path queries stage the tables in LDS and refuse scenes beyond 160 KiB with their own messages unless
 * the context was created with RT_FLAG_STREAM_QUERIES (below); shadow and bounce rays of a streamed frame test every object
 * (RT_FLAG_STREAM_CULL, below, culls the shadow rays' unit spheres by chunk). */
#define RT_FLAG_STREAM 8192u

/* Streamed queries: the queries for scenes of any size.  rt_render_gbuffer, rt_pick, rt_object_extents[_host],
 * rt_trace_rays[_host], rt_occluded_rays, rt_shade_rays[_host], rt_trace_paths[_host] and rt_pick_paths -- and through them
 * rt_render_gbuffer_multi, rt_object_extents_multi[_host] and rt_multi_query_ctx's context -- copy all class tables into one
 * workgroup's LDS and answer RT_ERR_SCENE from 2 561 spheres on.  Their streamed twins (rt_stream_queries.hip) read the tables as the
 * streamed frame kernel does, 64 entries at a time through a wave-private LDS slice.  The rule is one decision per context, made in
 * rt_create and never revisited (rt_set_scene cannot change the layout); rt_get_streamed_queries reports it:
 *     streamed queries = RT_FLAG_STREAM_QUERIES && (rt_get_streamed || the G-buffer's tables exceed 160 KiB of LDS)
 * False: every entry point is what it is without the flag, refusals and messages included -- the flag alone costs a small scene
 * nothing.  True: every entry point above launches its streamed kernel and none refuses for size.  RT_FLAG_STREAM | RT_FLAG_STREAM_QUERIES
 * forces the streamed query kernels on a scene of any size.
 * Accuracy: in strict contexts every streamed entry point returns bit for bit what the staged one returns wherever both run, for every
 * degree (the same chunks, the same chunk bodies, an acceptance rule that does not depend on the order within a tie); within one
 * context, RT_FLAG_FAST included, rt_pick is the planes' entry, rt_object_extents the reduction of the planes, and plane 0 of
 * rt_pick_paths is rt_pick for degree <= 2 -- the promises of the staged family.  RT_FLAG_FAST is its own arithmetic.
 * The flag combines with every other RT_FLAG_* and has no refusal of its own; through rt_create_multi it reaches every context.
 * Unchanged: adaptive supersampling and RT_FLAG_SSAA_GEOMETRY keep their rt_create refusals for large scenes (RT_FLAG_STREAM_ADAPTIVE,
 * below, lifts them), the G-buffer family
 * keeps refusing supersampling contexts, and RT_FLAG_COUNT books none of these rays.  Argument checks, alignment and overlap
 * refusals, `ms` and capturability are those of the staged calls, with the same number of graph nodes per call.
 * (16384 = 0x4000 is also the value of RT_ABI_DIAGNOSTIC; that define lives in the version word rt_abi_version returns, not in
 * rt_config.flags: the two never meet.) */
#define RT_FLAG_STREAM_QUERIES 16384u

/* Streamed adaptive supersampling: RT_FLAG_SSAA_ADAPTIVE, with or without RT_FLAG_SSAA_GEOMETRY, for scenes of
 * any size.  The refine and halo passes of an adaptive frame copy every object record and a culling entry into one workgroup's LDS
 * (288 bytes per object: RT_ERR_SCENE from 569 objects on), the G pass of RT_FLAG_SSAA_GEOMETRY all class tables (from 2 561 spheres
 * on), and without RT_FLAG_SIMPLE the plain pass must fit the wavefront kernel (from 1 685 spheres on).  Their streamed twins
 * (rt_stream_adaptive.hip; the G-buffer kernel of rt_stream_queries.hip) read the tables 64 entries at a time through a wave-private LDS
 * slice.  The rule is one decision per context, made in rt_create and never revisited (rt_set_scene cannot change the layout);
 * rt_get_streamed_adaptive reports it:
 *     streamed adaptive = RT_FLAG_SSAA_ADAPTIVE && RT_FLAG_STREAM_ADAPTIVE &&
 *                         (RT_FLAG_STREAM || (!RT_FLAG_SIMPLE && the wavefront kernel's LDS exceeds 160 KiB)
 *                          || n_objects * 288 bytes exceed 160 KiB || (RT_FLAG_SSAA_GEOMETRY && the G-buffer's tables exceed 160 KiB))
 * False: the context is, call for call and message for message, what it is without the flag -- the three size refusals keep their
 * order and texts, and the flag alone costs a small scene nothing.  True: none of the three refuses, nor does the refusal of
 * RT_FLAG_STREAM with RT_FLAG_SSAA_ADAPTIVE.  RT_FLAG_STREAM | RT_FLAG_SSAA_ADAPTIVE | RT_FLAG_STREAM_ADAPTIVE forces the streamed
 * passes on a scene of any size.
 * Definition: the frame of RT_FLAG_SSAA_ADAPTIVE / RT_FLAG_SSAA_GEOMETRY unchanged -- the same refine(x, y), tau, geo and
 * 8-neighbourhood; output = the resolve of S where refined, else P.  P is what rt_render of a k = 1 context with otherwise equal flags
 * stores: the plain pass keeps the rule of rt_get_streamed (at 569 ... 1 684 spheres it is still the wavefront kernel).  S(X, Y) is
 * the colour of sample (X, Y) of the k-times finer grid by the arithmetic of the streamed frame kernel, i.e. of rt_shade_rays, resolved
 * with the fixed pairwise tree, times 1/k^2, quantised for RGBA8 as everywhere.  obj / N of RT_FLAG_SSAA_GEOMETRY are bit for bit what
 * rt_render_gbuffer / rt_pick report on a streamed-queries context (the same kernel computes them; where that context's
 * RT_FLAG_STREAM_CULL_PIXELS decision is true its two calls run the culling twin while the G pass keeps the streamed kernel, and the
 * equality holds by that flag's rule -- the same spheres tested, an order-independent acceptance -- not by identity of kernel).
 * Accuracy: in strict contexts, for surfaces of degree <= 2, the frame and rt_get_ssaa_refined are bit-identical to the CPU reference's
 * composition and to the context without the flag wherever that one is accepted; for every degree tau < 0 gives bit for bit the frame of
 * a RT_FLAG_STREAM | RT_FLAG_SSAAk context.  RT_FLAG_FAST is its own arithmetic, held to 1e-5 relative like every RT_FLAG_FAST frame.
 * Unchanged: rt_set_ssaa_threshold, rt_set_ssaa_geometry, rt_get_ssaa_refined, both formats, ranks and bands (every rank's rows equal
 * the single context's), rt_pack_sparse, rt_set_scene, the multi-GPU layer (through rt_create_multi the flag reaches every context);
 * rt_render_sparse is refused where rt_get_streamed says 1 and is render + pack otherwise.  Nothing is read back and a frame is
 * capturable with ms == NULL.  Graph nodes per frame behind the plain pass: the halo kernel (world > 1), the list's memset, with
 * RT_FLAG_SSAA_GEOMETRY the G pass -- one node, two with world > 1 (planes, then the halo records; the staged pass is one or two as
 * well) --, the classifier, the refine kernel, and the pack of a sparse call.
 * Refused: RT_FLAG_STREAM_ADAPTIVE without RT_FLAG_SSAA_ADAPTIVE (RT_ERR_INVALID, before rt_create looks for a device); RT_FLAG_COUNT
 * on a context whose decision is true (RT_ERR_SCENE: the streamed passes book no counters); RT_FLAG_STREAM | RT_FLAG_COUNT stays
 * RT_ERR_INVALID.
 * Known limits: without RT_FLAG_STREAM_CULL sample rays and halo rays are not cone-culled (their waves are not 8 x 8 blocks), and shadow
 * and bounce rays test every object; with it, see "Culled streamed adaptive passes" below.  Out of scope: counters in streamed passes; the flag as a default; the G-buffer and picking
 * on supersampling contexts; degree-3 scene updates. */
#define RT_FLAG_STREAM_ADAPTIVE 32768u

/* Culled streamed frames: the streamed frame kernel stages every 64-entry chunk of the unit-sphere table for
 * every query, so a frame costs O(hits x lights x spheres).  With this flag the table is kept in a spatial order, every chunk has a
 * bounding sphere, and a query stages only the chunks whose bound the culling predicates of the wavefront kernel cannot rule out
 * (csrc/rt_stream_cull.hip).  (Bits 0x10000 .. 0x40000 are rt_create_multi's RT_MULTI_*.)  One decision per context, made in rt_create
 * and never revisited (rt_set_scene cannot change the layout); rt_get_stream_cull reports it:
 *     stream cull = RT_FLAG_STREAM_CULL && rt_get_streamed && culling is on (no RT_FLAG_NOCULL, at least 4 unit spheres with a radius)
 * False: the context is, call for call and byte for byte, what it is without the flag.  True: rt_create puts the unit-sphere table of
 * the scene blob into a deterministic order -- spheres with a bounding radius first, by a Morton key of their centres (21 bits per axis
 * over the box of those centres, ties by object index), the others behind them in index order; `orig` carries the object index as ever
 * and nothing else in the blob moves -- and keeps one bound per chunk in an allocation of its own (rt_debug_stream_bounds).  The order
 * is part of the layout and stays: after rt_set_scene the device holds, byte for byte, what rt_create packs for the new scene UNDER THE
 * CONTEXT'S ORDER, and the bounds of the rebuilt chunks (the update kernel forms them with rt_create's own function).
 * Culled: the primary rays of an 8 x 8 block stage only the chunks whose bound reaches into the block's cone; the shadow rays of a
 * wave's hits towards one light stage only the chunks whose bound can block a ray from the ball around those hits, and sweep only the
 * entries of a staged chunk that can.  Not culled: a segment with a non-finite hit point; a directional light with |d|^2 <= 1e-7;
 * rays with components beyond 1e100 (they take the dense path over all objects); general quadrics, planes and degree-3 objects, which
 * are streamed in full; the nearest-hit queries of bounce rays (segments >= 1) unless RT_FLAG_STREAM_CULL_BOUNCE says otherwise.
 * Results are unchanged by definition: the frame is RT_FLAG_STREAM's frame.  Strict contexts: bit for bit, both formats, every degree.
 * RT_FLAG_FAST: the same arithmetic per tested object; only the set of tested objects shrinks, and a dropped object's answer could not
 * have been accepted.  The nearest-hit rule does not depend on the table's order (nearest, lowest object index on a tie), so every
 * other reader of the blob -- the query kernels, staged or streamed, and the adaptive passes -- returns what it returns without the flag.
 * Culled streamed adaptive passes (csrc/rt_stream_cull_adaptive.hip): no flag of its own -- RT_FLAG_STREAM_CULL |
 * RT_FLAG_STREAM_ADAPTIVE says what the caller wants.  One more decision per context, made in rt_create and never revisited;
 * rt_get_stream_cull_adaptive reports it:
 *     stream cull adaptive = rt_get_stream_cull && rt_get_streamed_adaptive && at least 2 chunks (65 unit spheres)
 * False: the halo and refine passes are RT_FLAG_STREAM_ADAPTIVE's, launch for launch.  True: both are the culling twin of that kernel.
 * The sample rays (and halo centre rays) of a wave all leave the frame's origin: the wave forms a cone from its lanes' own directions
 * -- the axis is the direction of the used lane nearest their mean, the opening the minimum over all used lanes -- and stages only the
 * chunks whose bound reaches into it; the shadow rays of every segment are culled as in the frame kernel, from the ball around the
 * wave's hit points.  Not culled: what the frame kernel does not cull (above), and a wave with a ray beyond 1e100.  Results are
 * unchanged by definition: strict and RT_FLAG_FAST frames and rt_get_ssaa_refined are bit for bit those of the same context without
 * RT_FLAG_STREAM_CULL, every degree, both formats, every rank.  Graph nodes per frame, capturability, ms, rt_render_sparse's rules and
 * rt_set_scene are those of RT_FLAG_STREAM_ADAPTIVE (the update kernel already rebuilds the bounds).  The two-chunk floor: with a single
 * chunk the chunk level can remove nothing and is paid per query.
 * Known limits of the culled adaptive passes (measured; 1080p, k = 4, tau = 1/32): a k = 4 wave holds four
 * pixels of the refine list, usually from blocks that are not neighbours, so its cone is wide: at 10 000 spheres it still stages 45 of
 * 157 chunks per wave, the frame takes 0.29 x the unculled passes' time (0.62 x at 1 685 spheres) and, at 4.7 % refined, is still slower
 * than the culled full RT_FLAG_SSAA4 frame (16.0 against 6.7 ms).  At 65 spheres (two chunks) nothing is gained: 1.003 x in one run,
 * beyond the 0.2 us spread of the unculled series, 0.999 x in another.
 * No refusal of its own; combines with every flag; through rt_create_multi it reaches every context.
 * Known limits: the bounds are spheres around Morton runs of 64 entries, not a hierarchy: a scene whose spheres all overlap gains
 * nothing and pays one decision per chunk, and so does a scene of a single chunk (measured: 20spheres with its 19 lights takes 1.67 x
 * the time of RT_FLAG_STREAM alone; the 1 685- and 10 000-sphere fields of DESIGN.md section 25 take 0.215 x and 0.026 x).  Bounce
 * rays: RT_FLAG_STREAM_CULL_BOUNCE below; caller-supplied rays: RT_FLAG_STREAM_CULL_RAYS below; the pixel queries:
 * RT_FLAG_STREAM_CULL_PIXELS below; a second level over the chunk bounds: RT_FLAG_STREAM_CULL_GROUPS below.  Out of scope: bounds for the
 * other classes; reordering the refine list for tighter wave cones; counters (RT_FLAG_COUNT) in streamed passes; the flag as a default. */
#define RT_FLAG_STREAM_CULL 524288u

/* Culled bounce rays (csrc/rt_stream_cull_bounce.hip): in a culled streamed frame the nearest-hit query of a bounce
 * ray (segments >= 1) still sweeps the whole unit-sphere table, so a frame with mirrors is back at O(hits x spheres).  With this flag
 * every lane asks about its OWN ray and each chunk bound (csrc/rt_ray_bound.hpp: sphere_relevant for the half-line from the ray's origin
 * along its direction, the ball shrunk to radius 0), the wave stages a chunk only if some lane in use reaches its bound, and sweeps it for
 * those lanes alone.  One decision per context, made in rt_create and never revisited (rt_set_scene keeps both the mirrors' presence and
 * the chunk layout); rt_get_stream_cull_bounce reports it:
 *     stream cull bounce = RT_FLAG_STREAM_CULL_BOUNCE && rt_get_stream_cull && some object has a reflection ratio > 1e-7
 *                          && max_reflections >= 1 && at least 2 chunks (65 unit spheres)
 * False: the context is, launch for launch and byte for byte, the context without the flag; the flag without RT_FLAG_STREAM_CULL is simply
 * false.  There is no refusal of its own, and the flag combines with every other.  True: rt_render launches
 * stream_cull_bounce_frame_kernel, the culled frame kernel with that one query exchanged; primary and shadow rays are culled as before.
 * Not culled for: a ray with |d|^2 <= 1e-7 or not finite (the reference's linear branch is not geometry); a ray with a component
 * beyond 1e100 (it takes the dense path over all objects); a chunk whose bound is +inf; the other classes' tables.
 * Results are unchanged by definition: the frame is RT_FLAG_STREAM's frame.  Strict contexts: bit for bit, every degree, both formats.
 * RT_FLAG_FAST: bit for bit the unflagged FAST frame (the same arithmetic per tested object).  Graph nodes per frame, ms, capturability,
 * RT_FLAG_SSAA2/4, ranks, rt_pack_sparse and rt_set_scene are those of RT_FLAG_STREAM_CULL.  The halo and refine passes of adaptive
 * frames and the query kernels are not touched.  Through rt_create_multi the flag reaches every context.  All four instantiations of
 * both builds fit two waves per SIMD without a spill (the strict one for general quadrics plus degree 3 at exactly 256 VGPRs), so no
 * scene is excluded.
 * Known limits: the chunk level works on the union over a wave's 64 lanes, and the bounce rays of a block are not coherent -- a chunk is
 * staged as soon as ONE lane reaches its bound; chunks are not pruned against the nearest hit found so far (no best_t test, no near-to-far
 * order), so a ray pays for every chunk along its whole half-line; there is no per-entry level inside a staged chunk; every lane pays one
 * verdict per chunk and query, which a scene of few chunks does not earn back.  Measured (DESIGN.md section 27,
 * profiles/stream_cull_bounce.txt; MI355X, 1920 x 1080, strict RGBA32F, the mirrored sphere field with two bounces, against
 * RT_FLAG_STREAM | RT_FLAG_STREAM_CULL): 10 000 spheres 10 660 -> 4 467 us (0.42 x), 1 685 spheres 812 -> 680 us (0.84 x), 65 spheres
 * 409.5 -> 406.8 us; with spheres 20 pixels across 0.71 x, 0.88 x and 1.002 x (1.1 us more, beyond the 0.8 us spread).  At 10 000
 * spheres a lane reaches 12 % of the bounds ([3] / [2]) while the wave stages 24 % of them ([1] / [0]); at 65 spheres both are one half.
 * Out of scope: pruning by best_t and an ordered traversal; a per-entry level; the bounce rays of the adaptive and query kernels;
 * bounds for the other classes; a hierarchy over the bounds; the flag as a default or as part of
 * RT_FLAG_STREAM_CULL. */
#define RT_FLAG_STREAM_CULL_BOUNCE 1048576u

/* Culled ray queries (csrc/rt_stream_cull_rays.hip): on a streamed-queries context rt_trace_rays,
 * rt_occluded_rays, rt_shade_rays, rt_trace_paths, rt_pick_paths and the _host forms stage and sweep every chunk of the unit-sphere table
 * for every wave and every segment, shadow rays included: O(rays x spheres).  With this flag every lane asks about its OWN ray and each
 * chunk bound (csrc/rt_ray_bound.hpp, the predicate of RT_FLAG_STREAM_CULL_BOUNCE, about the ray's whole half-line), the wave stages a
 * chunk only if some lane in use reaches its bound, and sweeps it for those lanes alone; an occlusion query stops behind the chunk that
 * blocks its last undecided lane.  One decision per context, made in rt_create and never revisited (rt_set_scene rebuilds the bounds and
 * keeps the layout); rt_get_stream_cull_rays reports it:
 *     stream cull rays = RT_FLAG_STREAM_CULL_RAYS && rt_get_stream_cull && rt_get_streamed_queries && at least 2 chunks (65 unit spheres)
 * False: the context is, launch for launch and byte for byte, the context without the flag.  There is no refusal of its own, and the flag
 * combines with every other.  True: the five entry points launch the culling twins of the streamed ray kernels (the same arguments,
 * grid, loads and stores; one graph node as before).  The shading loop of rt_shade_rays culls the nearest hit of every segment and every
 * shadow ray as the ray it is; t_max of rt_occluded_rays bounds the roots, not the verdicts.
 * Not culled for: a ray with |d|^2 <= 1e-7 or not finite (the reference's linear branch is not geometry) -- its WAVE then stages every
 * chunk; a ray with a component beyond 1e100 (it takes the dense path over all objects); a chunk whose bound is +inf; the other classes'
 * tables; the pixel queries (rt_render_gbuffer, rt_pick, rt_object_extents), which have a flag of their own (RT_FLAG_STREAM_CULL_PIXELS below).
 * Results are unchanged by definition: every output is bit for bit that of the same context without the flag, strict and RT_FLAG_FAST,
 * every degree.  ms, capturability, ranks and rt_set_scene are those of the streamed queries.  Through rt_create_multi the flag reaches
 * every context.  All sixteen instantiations of both builds fit two waves per SIMD without a spill (at most 216 VGPRs), so no scene is
 * excluded.
 * Known limits: the chunk level works on the union over a wave's 64 lanes, a wave being 64 CONSECUTIVE rays of the caller's array -- rays
 * in no spatial order gain little (DESIGN.md section 29 measures row order against a shuffle); no best_t pruning and no near-to-far order;
 * no per-entry level inside a staged chunk; every lane pays one verdict per chunk and query, which a scene of few chunks does not earn
 * back.  Measured (profiles/stream_cull_rays.txt; MI355X, strict, the 1920 x 1080 frame's own primary rays as the
 * rays, against the same context without the flag): in row order 10 000 spheres rt_trace_rays 21 764 -> 4 165 us, rt_shade_rays 61 732 ->
 * 12 204 us (0.19 - 0.25 x over the four entry points), 1 685 spheres 0.41 - 0.51 x; the same rays shuffled stage 98 - 100 % of the
 * chunks and take 1.13 - 1.32 x in rt_trace_rays, rt_occluded_rays and rt_trace_paths while rt_shade_rays still gains (0.55 - 0.85 x);
 * at 65 spheres (two chunks) every entry point is slower, 1.13 - 1.29 x.
 * Out of scope: bounds for the other classes; a hierarchy over the bounds; the flag as a default. */
#define RT_FLAG_STREAM_CULL_RAYS 2097152u

/* Culled pixel queries (csrc/rt_stream_cull_pixels.hip): on a streamed-queries context rt_render_gbuffer, rt_pick
 * and rt_object_extents (and through them rt_render_gbuffer_multi, rt_object_extents_multi[_host], mi355rt_update_pick and
 * mi355rt_update_extents) stage and sweep every chunk of the unit-sphere table for every 8 x 8 block: O(pixels x spheres).  With this flag
 * a wave asks sphere_in_cone -- the predicate its block's cone already asks about every sphere -- about the chunk bounds first, lane =
 * chunk, and stages only the chunks whose bound reaches into the cone; inside a staged chunk the per-sphere cone runs as before.  One
 * decision per context, made in rt_create and never revisited (rt_set_scene rebuilds the bounds and keeps the layout);
 * rt_get_stream_cull_pixels reports it:
 *     stream cull pixels = RT_FLAG_STREAM_CULL_PIXELS && rt_get_stream_cull && rt_get_streamed_queries && at least 2 chunks (65 unit spheres)
 * False: the context is, launch for launch and byte for byte, the context without the flag.  There is no refusal of its own, and the flag
 * combines with every other.  True: the entry points launch the culling twins of the streamed pixel kernels (the same arguments, grid,
 * loads and stores; graph nodes as before: planes 1, picks 1, extents 2).
 * Not culled: the other classes' tables (general quadrics, planes, degree 3), streamed in full; a chunk whose bound is +inf (a sphere
 * without a radius in it); picks -- rt_pick's pixels are unrelated, so its waves run the same loop under a cone that culls nothing and
 * stage every chunk; the G pass of an RT_FLAG_SSAA_GEOMETRY frame, which keeps the streamed kernels.
 * Results are unchanged by definition: a skipped bound implies that every member is skipped by the same predicate, and the per-sphere cone
 * skips exactly those members already, so the spheres tested are the unflagged kernels' and the acceptance rule does not depend on their
 * order (nearest, lowest object index on a tie).  Every output is bit for bit that of the same context without the flag, strict and
 * RT_FLAG_FAST, every degree; a picked pixel is the planes' entry (one kernel, two launch modes, as before), and extents are the
 * reduction of the planes.  ms, capturability, ranks and rt_set_scene are those of the streamed queries.  Through rt_create_multi the
 * flag reaches every context.  All eight instantiations of both builds fit two waves per SIMD without a spill, so no scene is excluded.
 * Known limits: picks gain nothing from culling and pay one verdict per chunk; a scene of two chunks can remove little and pays the
 * verdicts per block; chunks are not pruned against the nearest hit found so far and not visited near to far; the bounds are spheres
 * around Morton runs of 64 entries, not a hierarchy.  Measured (profiles/stream_cull_pixels.txt; MI355X,
 * 1920 x 1080, strict, the sphere field, against the same context without the flag): 10 000 spheres rt_render_gbuffer 1 112 -> 157 us
 * (0.14 x), rt_object_extents 1 134 -> 172 us (0.15 x), 11 % of the chunks staged; 1 685 spheres 203 -> 73 us and 204 -> 79 us
 * (0.36 x, 0.39 x); 65 spheres (two chunks) both inside the unflagged series' spread (27.2 / 27.3 us, 31.6 / 31.5 us).  rt_pick of 1
 * and of 4 096 pixels stages every chunk and saves not one test; by the host's clock around the blocking call it measured 0.91 - 0.97 x
 * at all three sizes (1 630 -> 1 481 us for one pixel at 10 000 spheres).  That figure is unexplained -- the two kernels' code was not
 * compared -- and promises nothing: expect the unflagged time, neither a gain nor a guaranteed absence of overhead.
 * Out of scope: per-lane culling for picks; the adaptive G pass; best_t pruning, near-to-far order, a hierarchy over the bounds; bounds
 * for the other classes; the flag as a default.  Supersampling contexts stay refused by the G-buffer family as before. */
#define RT_FLAG_STREAM_CULL_PIXELS 4194304u

/* Re-sorting a culled scene (csrc/rt_reorder_scene.hip): RT_FLAG_STREAM_CULL and the flags built on it cull because the
 * unit-sphere table is in Morton order, chosen once by rt_create; rt_set_scene keeps that order, so the chunks of a scene whose spheres
 * mix grow towards the whole field and the frames, still correct, again stage every chunk.  With this flag rt_reorder_scene ("Scene
 * updates") puts the table the device holds into the order a fresh rt_create would choose and rebuilds the chunk bounds, on the device and
 * in stream order.  One decision per context, made in rt_create and never revisited; rt_get_stream_cull_reorder reports it:
 *     reorder = RT_FLAG_STREAM_CULL_REORDER && rt_get_stream_cull
 * False: the context is, call for call and byte for byte, the context without the flag: no extra allocation, and rt_reorder_scene returns
 * RT_OK and enqueues nothing.  True: rt_create also allocates the reorder work space (sized from the number of unit spheres alone: 96
 * bytes per sphere and the sort's histogram tables; freed by rt_destroy).  The flag combines with every other and reaches every context
 * of rt_create_multi.  No result depends on the table's order ("Order"), so no frame and no query changes.
 * Diagnostics: MI355RT_REORDER_MAX_GRID=<1 .. 65535> in the environment at rt_create caps the workgroups of every launch of
 * rt_reorder_scene (default: four per compute unit); any other value is refused (RT_ERR_INVALID).  Results do not depend on it. */
#define RT_FLAG_STREAM_CULL_REORDER 8388608u

/* Grouped chunk bounds (csrc/rt_stream_cull_groups.hip): a culled streamed frame asks one verdict per chunk bound --
 * per 8 x 8 block for the primary rays, per (wave, light) for the shadow rays and, with RT_FLAG_STREAM_CULL_BOUNCE, per lane and bounce
 * ray -- so its cost still grows with the number of chunks: at 100 000 spheres 1 563 bounds per query, almost all of them nowhere near
 * it.  With this flag the context keeps a second level: a GROUP is 64 consecutive chunks (4 096 entries of the ordered unit-sphere table,
 * a compact cell of the Morton order), and its bound is formed from the group's chunk bounds by the function that forms a chunk bound
 * from its spheres (csrc/rt_scene_pack.hpp, pack_chunk_bound, orig = the group's index; a group with an unbounded chunk is unbounded and
 * never skipped).  That function's proof -- bound skipped => member skipped by its own predicate, by a margin that dwarfs rounding --
 * asks of a member a centre, an r and an inv_r, which a chunk bound has: a skipped group implies 64 skipped chunk bounds, and those every
 * sphere.  One decision per context, made in rt_create and never revisited (rt_set_scene and rt_reorder_scene keep the chunk layout);
 * rt_get_stream_groups reports it:
 *     stream groups = RT_FLAG_STREAM_CULL_GROUPS && rt_get_stream_cull && at least 2 groups (65 chunks: 4 097 unit spheres)
 *                     && the kernel is built (below: every context but one diagnostic combination)
 * False: the context is, launch for launch and byte for byte, the context without the flag; the flag without RT_FLAG_STREAM_CULL is simply
 * false.  There is no refusal of its own, and the flag combines with every other.  True: rt_render launches
 * stream_cull_groups_frame_kernel.  Primary and shadow queries: per block of 64 groups lane j asks the query's own predicate (the block's
 * cone; the ball of the wave's hits and the light) about group bound j, one ballot is the mask of the groups to enter, and only those run
 * the chunk loop of RT_FLAG_STREAM_CULL for their 64 chunks.  Bounce rays, where rt_get_stream_cull_bounce is 1: every lane asks about its
 * own ray and the group bound, and the 64 chunks of a group that no lane in use reaches are passed over; where it is 0 bounce rays keep
 * the full sweep.  The group bounds follow the chunk bounds: rt_set_scene and rt_reorder_scene each enqueue one more small kernel behind
 * their own (one more graph node each; both stay capturable, a refused update recomputes the same bytes).
 * Results are unchanged by definition: the chunks staged, the order they are staged in and the place of the occlusion early-out are those
 * of the same context without the flag, so every frame is that context's bit for bit -- strict and RT_FLAG_FAST, both formats, every
 * degree, rank and RT_FLAG_SSAA2/4 mode.  ms, capturability, ranks and rt_pack_sparse are those of RT_FLAG_STREAM_CULL.  Through
 * rt_create_multi the flag reaches every context.  Work words: with MI355RT_STREAM_CULL_STATS=1 rt_debug_stream_cull and
 * rt_debug_stream_cull_bounce count what the kernel now asks and stages -- the staged words are those of the unflagged context, the
 * decision words ([0], [2]; bounce [0], [2]) count only the chunk bounds of entered groups --, and rt_debug_stream_groups has the group
 * verdicts.  The fifteen instantiations of each build that are built fit two waves per SIMD without a spill (at most 254 VGPRs; the eight
 * that do not count at most 235).  Not built: the kernel that COUNTS and culls bounce rays for a scene with both general quadrics and
 * degree-3 objects, which does not fit two waves per SIMD in either build.  The decision is false for the contexts that would need it:
 * such a scene, rt_get_stream_cull_bounce 1 and MI355RT_STREAM_CULL_STATS=1 in the environment at rt_create.  Without the diagnostic
 * switch no scene is excluded.
 * Known limits: three groups cannot remove much and cost one more verdict per query; groups are Morton runs, and a run that straddles two
 * clusters has a bound around both; on a scene with both general quadrics and degree-3 objects and culled bounce rays the diagnostic switch
 * MI355RT_STREAM_CULL_STATS=1 makes the decision false, so the work words of the grouped kernel that such a context runs WITHOUT the
 * switch cannot be read -- profile such a scene without RT_FLAG_STREAM_CULL_BOUNCE, or by time alone; every rt_set_scene and
 * rt_reorder_scene of a groups context is followed by one more small kernel (one thread per group, 128 dependent 64-byte loads long).
 * Measured (profiles/stream_cull_groups.txt; MI355X, 1920 x 1080, strict RGBA32F, the
 * sphere field, against the same context without the flag): A SMALL GAIN, 0.1 - 2.2 %.  10 000 spheres 945.4 -> 936.7 us, 100 000 spheres
 * 42 018 -> 41 966 us (inside the unflagged series' spread of 93 us), 400 000 spheres 218 601 -> 218 117 us, although there 82 % of the
 * primary and 57 % of the shadow chunk verdicts are gone: the time of a large scene is in the staged chunks of its shadow rays (768 million
 * entries decided per frame at 100 000 spheres), not in the verdicts.  The mirrored field with RT_FLAG_STREAM_CULL_BOUNCE, whose per-lane
 * loop pays most per chunk: 10 000 spheres 4 413 -> 4 318 us, 100 000 spheres 170 913 -> 168 008 us (37 % of the bounce chunk verdicts gone;
 * a wave's 64 bounce rays together still enter 62 % of the groups).  No case lost.  The group-bounds kernel adds 33 - 47 us to every
 * rt_set_scene and rt_reorder_scene, more than a frame gains below about 100 000 spheres.
 * Out of scope: the adaptive, ray-query and pixel-query culling kernels keep their chunk loops (on a groups context they run unchanged and
 * return the same bits); any fan-out other than 64; a third level; best_t pruning; the flag as a default. */
#define RT_FLAG_STREAM_CULL_GROUPS 16777216u

/* rt_config.format -- framebuffer pixel format */
#define RT_FMT_RGBA32F 0u     /* 4 x float per pixel, alpha 1.0: the un-quantised colours the CPU back end
                                 produces (src/update-cpu.cpp:128-131) plus an alpha lane for 16-byte stores */
#define RT_FMT_RGBA8 1u       /* iround(c*255) RGBA8, alpha 255: the wire format of src/update-cuda.cu:149-156 */

typedef struct rt_config {
    int32_t device;      /* HIP device ordinal, -1 = the calling thread's current device */
    uint32_t rank;       /* this context renders the row bands b with b % world == rank */
    uint32_t world;      /* number of row-band owners (1 = whole frame) */
    uint32_t band_rows;  /* rows per band, 0 = default (8) */
    uint32_t flags;      /* RT_FLAG_* */
    uint32_t format;     /* RT_FMT_* */
} rt_config;

/* Device-side work counters of the last RT_FLAG_COUNT render (definitions: SURVEY.md 8(d)). */
typedef struct rt_counters {
    uint64_t primary_rays;  /* one per pixel */
    uint64_t shadow_rays;   /* shadow_ray calls: hits x lights (light_impl.h:17) */
    uint64_t reflect_rays;  /* reflect_ray calls (light_impl.h:46) */
    uint64_t tests;         /* ray-surface tests = intersect_ray calls in the reference (surface_impl.h:21) */
    uint64_t hits;          /* nearest-hit records shaded (normal_vector calls, surface_impl.h:157) */
    uint64_t solves;        /* root solves (sqrt + division, or the cubic solver) actually executed */
    uint64_t tests_executed; /* t2,t1,t0 evaluations actually executed (differs from `tests`: no early break,
                                minus culled objects) */
    uint64_t cull_evals;    /* bounding-sphere culling decisions evaluated (one lane each) */
} rt_counters;

/* The work the PRODUCT build executes for the frame of the last RT_FLAG_COUNT render, split the way the flop accounting needs
 * it (bench.py multiplies each entry with the cost of that unit, counted by tools/count_flops.cpp over the kernel's own math).
 * (A counting render itself traces more shadow rays than the product build -- it needs every first blocker's index for
 * rt_counters.tests -- but counts as executed only what the product build executes.) */
typedef struct rt_counters_detail {
    uint64_t tests_executed[4]; /* per surface class: unit sphere, other quadric, plane, cubic */
    uint64_t solves[3];         /* root solves per class: unit sphere, other quadric, plane (cubic: cubic_branch) */
    uint64_t cull_evals[5];     /* culling decisions: tile pyramid, primary cone, shadow phase directional / point light; records formed */
    uint64_t cubic_branch[4];   /* cubic tests by solver branch: Cardano, trigonometric, quadratic, linear / none (surface_impl.h:106-154) */
    uint64_t shadow_rays_traced; /* of rt_counters.shadow_rays: those not skipped because the hit faces away from the light */
    uint64_t hit_lights_shaded;  /* surface_color evaluations (light_impl.h:29) */
    uint64_t primary_rays_formed; /* pixels of the tiles that are actually traced (rt_counters.primary_rays counts every pixel) */
    uint64_t cubic_points;        /* (ABI 3) degree-3 surfaces: evaluations of F, grad F and the half Hessian at a ray origin (lanes); the data
                                   * of the frame's own origin comes from the host and is not counted */
    uint64_t cubic_refused;       /* (ABI 3) of tests_executed[3]: tests whose Taylor-form answer the guard refused (rt_math.hpp, cubic_guarded) and
                                   * that went through the reference's dense expansion and solver instead */
} rt_counters_detail;

typedef struct rt_ctx rt_ctx;
typedef struct rt_scene rt_scene;

int rt_abi_version(void);
const char *rt_last_error(void);
/* For layers built on this ABI (libmi355rt_multi.so): set the calling thread's error text. */
void rt_set_last_error(const char *message);

/* ---------------------------------------------------------------------------------------------------
 * Scene loading -- replaces Scene::load_from_file (include/scene.h:35, src/scene.cpp:154-203) and the
 * factories it calls (src/surface.cpp:4-60, src/light.cpp:4-26).  Same keys, defaults, validation and
 * error texts; own YAML-subset parser (yaml-cpp is not a dependency).
 * ------------------------------------------------------------------------------------------------- */
int rt_scene_load_file(const char *path, rt_scene **out);
/* Programmatic construction (Scene::Scene, src/scene.cpp:16-22; fov in DEGREES like the constructor). */
int rt_scene_new(uint32_t width, uint32_t height, double fov_deg, uint32_t max_reflections,
                 const float bg_color[3], rt_scene **out);
/* Object::Object (src/scene.cpp:9-14) with an explicit coefficient vector. */
int rt_scene_add_object(rt_scene *s, const double coefs[RT_NCOEF], float reflection_ratio, const float color[3]);
/* LightSource::directional / spherical (src/light.cpp:4-26); v = direction or position. */
int rt_scene_add_light(rt_scene *s, int is_spherical, float intensity, const double v[3], const float color[3]);
/* Surface factories, src/surface.cpp:4-60.  kind: 0 sphere(a=center,b[0]=radius) 1 plane(a=origin,b=normal)
 * 2 dingDong(a=origin) 3 clebsch 4 cayley. */
int rt_surface_make(int kind, const double a[3], const double b[3], double out_coefs[RT_NCOEF]);
/* Overrides of the public Scene fields (include/scene.h:19-22); bench configs use resolutions the YAML
 * files do not contain. */
int rt_scene_set_size(rt_scene *s, uint32_t width, uint32_t height);
int rt_scene_set_max_reflections(rt_scene *s, uint32_t max_reflections);
/* Borrowed view, valid until the scene is modified or freed. */
int rt_scene_get_desc(const rt_scene *s, rt_scene_desc *out);
void rt_scene_free(rt_scene *s);

/* The reference host's camera (src/ray-tracer.cpp:25-58): camera-to-world matrix
 * inverse(lookAt(pos, pos - direction(yaw, pitch), +y)), column-major, 16 doubles -- the argument update()
 * receives every frame.  Start-up pose (pos 0, yaw 90, pitch 0) is the identity to ~6e-17. */
int rt_camera_matrix(const double pos[3], double yaw_deg, double pitch_deg, double out_cam[16]);

/* ---------------------------------------------------------------------------------------------------
 * Rendering
 * ------------------------------------------------------------------------------------------------- */
/* Replaces init_update (include/update.h:6; src/update-cpu.cpp:22-43, src/update-cuda.cu:34-63):
 * copies the scene to the device, precomputes aspect and tan(fov/2), allocates the local framebuffer. */
int rt_create(rt_ctx **out, const rt_scene_desc *scene, const rt_config *cfg);

/* Replaces update (include/update.h:7; src/update-cpu.cpp:121-139, src/update-cuda.cu:160-190).
 *   cam     camera-to-world dmat4, column-major, 16 doubles (src/ray-tracer.cpp:54-58)
 *   dev_fb  device pointer receiving this rank's rows ([local_rows][width] pixels of cfg.format), or NULL for
 *           the context's own offscreen buffer
 *   stream  hipStream_t to launch on (NULL = default stream)
 *   ms      if non-NULL: the call synchronises and stores the device time of the render kernels in
 *           milliseconds (hipEvent pair, what the reference's update() returns); if NULL the call only
 *           enqueues work.
 * A context carries state from frame to frame on the device (which tiles had hits: the next frame starts those first; per-frame
 * tile words), so its frames run in the order they were issued: on one stream that is automatic, and when a call passes a
 * different stream than the previous one, that stream first waits for the previous frame (an event recorded behind every
 * render).  The state affects speed only, never the image.
 * Stream capture: with ms == NULL and the stream of the previous call, rt_render only enqueues (one kernel; the ordering event is
 * not recorded while the stream is capturing -- a context whose frames were captured must stay on that stream afterwards, a call on
 * another stream is refused with RT_ERR_INVALID), so a
 * sequence of K frames can be captured into one hipGraph and launched at once -- bench.py times its frames that way (the ~3 us the
 * command processor needs between two dependent launches disappear: 42 instead of 45 us per 1080p frame).  Every captured call
 * carries its own arguments (camera, launch-order generation, frame tag): launched once, in place of the K calls, the graph is
 * exactly those K frames; REPLAYING it renders correctly too but repeats frame tags and generations, i.e. without the benefit of
 * the ordering (use RT_FLAG_STATIC_ORDER for contexts whose graphs are replayed).  Tested (tests/test_graph_replay_gpu.py): a graph
 * may be replayed any number of times, also several graphs of one context in turn and with uncaptured frames in between, and the
 * counters and sparse messages of the frame that follows are unaffected. */
int rt_render(rt_ctx *ctx, const double cam[16], void *dev_fb, void *stream, float *ms);

/* Row ownership: number of local rows, and for local row i its global y (row 0 = bottom of the image,
 * src/update-cpu.cpp:125-131).  rt_max_local_rows is the maximum over all ranks (gather stride). */
int rt_local_rows(const rt_ctx *ctx, uint32_t *n_rows);
int rt_max_local_rows(const rt_ctx *ctx, uint32_t *n_rows);
int rt_row_map(const rt_ctx *ctx, uint32_t *rows /* [local_rows] */);
size_t rt_pixel_bytes(const rt_ctx *ctx);

/* Offscreen buffer of the context (device pointer) and a blocking copy of it to host memory. */
void *rt_device_fb(rt_ctx *ctx);
int rt_download(rt_ctx *ctx, void *host_dst, size_t bytes);

/* Root-side reassembly after the gather (the only collective of the path): `gathered` holds
 * [world][max_local_rows][width] pixels in rank order, `full` receives [height][width] pixels in row order.
 * Both are device pointers; enqueued on `stream`. */
int rt_assemble(rt_ctx *ctx, const void *gathered, void *full, void *stream);
/* rt_assemble for planes that are not frames (the G-buffer's object, t and normal planes; what a torch.distributed host calls after its
 * own gather): gathered + q * slot_stride_bytes = rank q's [max_local_rows][width] elements of elem_bytes (4, 8 or 16) each; full
 * receives [height][width] elements in row order.  Row ownership is the context's (band_rows, world), i.e. exactly the mapping of
 * rt_assemble.  Device pointers, enqueued on `stream`: one kernel (csrc/rt_planes.hip), elements moved as they are.  RT_ERR_INVALID,
 * before a device is looked for: NULL arguments, another elem_bytes, a stride smaller than one slot or not a multiple of elem_bytes,
 * pointers not aligned to elem_bytes, `full` overlapping `gathered`, and supersampling contexts (their row map is the output frame's,
 * as for rt_render_gbuffer, which refuses them too). */
int rt_assemble_planes(rt_ctx *ctx, const void *gathered, size_t slot_stride_bytes, void *full, uint32_t elem_bytes, void *stream);

/* Sparse transport of a frame (what `rt_assemble` does, with fewer bytes over the links): most 16x16 tiles of a
 * typical frame are pure background, so a rank may send only the others.  rt_pack_sparse turns this rank's rows
 * (dev_fb, or the context's own buffer if NULL) into a fixed-size message of rt_sparse_msg_bytes(format, capacity_tiles) bytes:
 *   uint32 { count, overflow, 0, 0 }, uint32 ids[capacity] (padded to 16 bytes), capacity x 256 pixels of the context's format
 *   (tile-major, 16 rows of 16 pixels: 1 KiB per RGBA8 tile, 4 KiB per RGBA32F tile; every tile starts 16-byte aligned);
 * `overflow` != 0 means more than capacity_tiles tiles had content (send the dense frame instead).  A tile is background when
 * every pixel is bit-equal to the background pixel: RGBA8 iround(bg_color * 255) with alpha 255, RGBA32F (bg_color, 1.0f) --
 * what the render kernels store where a primary ray hits nothing.  The root gathers the messages ([world][rt_sparse_msg_bytes]
 * in rank order) and rt_assemble_sparse rebuilds [height][width] pixels.
 * The reference has no counterpart (single GPU); the dense gather + rt_assemble stays the general path. */
size_t rt_sparse_bytes(uint32_t capacity_tiles); /* RGBA8 messages: rt_sparse_msg_bytes(RT_FMT_RGBA8, capacity_tiles) */
/* Message size for a pixel format (RT_FMT_*); no context needed.  0 for an unknown format. */
size_t rt_sparse_msg_bytes(uint32_t format, uint32_t capacity_tiles);
/* rt_render that writes such a message directly (tiles in which a primary ray hit something; background tiles are not
 * stored anywhere): one kernel instead of render + pack, and no local framebuffer.  Arguments as rt_render.  Not with
 * RT_FLAG_SIMPLE.  (It renders with the general schedule: scenes the wave-per-block one would take render slower this way than
 * with rt_render + rt_pack_sparse.) */
int rt_render_sparse(rt_ctx *ctx, const double cam[16], void *dev_msg, uint32_t capacity_tiles, void *stream, float *ms);
int rt_pack_sparse(rt_ctx *ctx, const void *dev_fb, void *dev_msg, uint32_t capacity_tiles, void *stream);
int rt_assemble_sparse(rt_ctx *ctx, const void *gathered_msgs, uint32_t capacity_tiles, void *full, void *stream);
/* The same without repainting the whole frame every time: `full` and `stamps` (rt_sparse_stamp_bytes(ctx) bytes of device
 * memory owned by the caller, one pair per output buffer) carry over from the previous call on that buffer; only tiles an
 * earlier frame delivered and this one did not are painted back to the background.  frame_tag: 0 on the first call for a
 * buffer (paints everything, clears the stamps), afterwards any value in [1, 0xFFFFFFFE] that differs from the previous
 * call's. */
size_t rt_sparse_stamp_bytes(rt_ctx *ctx);
int rt_assemble_sparse_incremental(rt_ctx *ctx, const void *gathered_msgs, uint32_t capacity_tiles, void *full, void *stamps, uint32_t frame_tag,
                                   void *stream);

/* Counters of the last render done with RT_FLAG_COUNT. */
int rt_get_counters(rt_ctx *ctx, rt_counters *out);
int rt_get_counters_detail(rt_ctx *ctx, rt_counters_detail *out); /* wavefront kernel only */

/* Diagnostics: the raw device counter block (32 words).  Words 0-7 are rt_counters; words 8+ are per-phase
 * wave-cycle totals that only a library built with `make STAMPS=1` fills in. */
int rt_debug_counters(rt_ctx *ctx, uint64_t out[32]);
/* Diagnostics (`make STAMPS=1` + MI355RT_DEBUG_COUNTERS=1 only): the last frame's per-wave rows of 16 words -- 0-11 cycles per phase,
 * 12 / 13 a 100 MHz clock at the wave's start / end; row = workgroup * 4 + wave.  out = NULL: only the row count. */
int rt_debug_stamp_rows(rt_ctx *ctx, uint64_t *out, size_t max_rows, size_t *n_rows);
/* Diagnostics: the render kernel's box helper run alone, one wave of 64 lanes per entry (csrc/rt_wave_box.hpp: the FP32 bounding box of a
 * block's or a chunk's hit points, which feeds the conservative culling of shadow tests).  All four arrays are host memory: pts =
 * [n_waves][64][3] doubles, lane l's point; use_masks = [n_waves], bit l set: lane l's point counts; out = [n_waves][6] floats: lox, hix, loy,
 * hiy, loz, hiz -- per axis the minimum over the counted lanes of the largest float <= the coordinate and the maximum of the smallest float
 * >= it, taken as fminf / fmaxf take them (a NaN coordinate drops out); (+inf, -inf) where no lane counts.  The context only names the device
 * and the stream (that of its last call); nothing of it is read or changed.  The call copies in, runs one small kernel, copies out and
 * waits.  RT_ERR_INVALID for a NULL argument, for n_waves == 0 or > 65536, and while the context's stream is capturing. */
int rt_debug_wave_box(rt_ctx *ctx, const double *pts, const uint64_t *use_masks, uint32_t n_waves, float *out);

/* RT_FLAG_SSAA_ADAPTIVE contexts only (RT_ERR_INVALID otherwise; a NaN tau is refused too).  The threshold applies from the next
 * rt_render on; it is a kernel argument, so a frame captured into a graph keeps the tau it was captured with. */
int rt_set_ssaa_threshold(rt_ctx *ctx, float tau);
/* RT_FLAG_SSAA_GEOMETRY contexts only (RT_ERR_INVALID for a NULL context, a context without the flag and a NaN min_cos): the normal
 * threshold c of the geometric term, default -inf (object ids only).  Like tau it applies from the next rt_render on and is a kernel
 * argument, so a frame captured into a graph keeps the value it was captured with. */
int rt_set_ssaa_geometry(rt_ctx *ctx, float min_cos);
/* The number of refined pixels of this context's last frame (waits for that frame). */
int rt_get_ssaa_refined(rt_ctx *ctx, uint64_t *pixels);
/* Streamed frames (RT_FLAG_STREAM above): *streamed = 1 where rt_render is the streamed kernel, else 0. */
int rt_get_streamed(const rt_ctx *ctx, uint32_t *streamed);
/* Streamed queries (RT_FLAG_STREAM_QUERIES above): *streamed = 1 where the query entry points launch their streamed kernels, else 0.
 * RT_ERR_INVALID for a NULL argument, before a device is looked for. */
int rt_get_streamed_queries(const rt_ctx *ctx, uint32_t *streamed);
/* Streamed adaptive supersampling (RT_FLAG_STREAM_ADAPTIVE above): *streamed = 1 where the halo, G and refine passes of rt_render are
 * the streamed kernels, else 0.  RT_ERR_INVALID for a NULL argument, before a device is looked for. */
int rt_get_streamed_adaptive(const rt_ctx *ctx, uint32_t *streamed);
/* Culled streamed frames (RT_FLAG_STREAM_CULL above): *on = 1 where rt_render culls whole chunks of the unit-sphere table, else 0.
 * RT_ERR_INVALID for a NULL argument (before a device is looked for). */
int rt_get_stream_cull(const rt_ctx *ctx, uint32_t *on);
/* Culled streamed adaptive passes (RT_FLAG_STREAM_CULL above): *on = 1 where the halo and refine passes of rt_render cull whole chunks
 * of the unit-sphere table (rt_get_stream_cull && rt_get_streamed_adaptive && at least two chunks), else 0.  RT_ERR_INVALID for a NULL
 * argument (before a device is looked for). */
int rt_get_stream_cull_adaptive(const rt_ctx *ctx, uint32_t *on);
/* Culled bounce rays (RT_FLAG_STREAM_CULL_BOUNCE above): *on = 1 where rt_render culls the unit-sphere chunks of its bounce rays per ray,
 * else 0.  RT_ERR_INVALID for a NULL argument (before a device is looked for). */
int rt_get_stream_cull_bounce(const rt_ctx *ctx, uint32_t *on);
/* Grouped chunk bounds (RT_FLAG_STREAM_CULL_GROUPS above): *on = 1 where rt_render asks a second level of bounds, one per 64 chunk
 * bounds, before the chunk bounds, else 0.  RT_ERR_INVALID for a NULL argument (before a device is looked for). */
int rt_get_stream_groups(const rt_ctx *ctx, uint32_t *on);
/* Culled ray queries (RT_FLAG_STREAM_CULL_RAYS above): *on = 1 where rt_trace_rays, rt_occluded_rays, rt_shade_rays, rt_trace_paths and
 * rt_pick_paths cull the unit-sphere chunks per caller-supplied ray, else 0.  RT_ERR_INVALID for a NULL argument (before a device is
 * looked for). */
int rt_get_stream_cull_rays(const rt_ctx *ctx, uint32_t *on);
/* Culled pixel queries (RT_FLAG_STREAM_CULL_PIXELS above): *on = 1 where rt_render_gbuffer, rt_pick and rt_object_extents cull the
 * unit-sphere chunks by the block's cone, else 0.  RT_ERR_INVALID for a NULL argument (before a device is looked for). */
int rt_get_stream_cull_pixels(const rt_ctx *ctx, uint32_t *on);

/* ---------------------------------------------------------------------------------------------------
 * G-buffer: what is under a pixel (object, depth, normal of the PRIMARY hit) and pixel picking
 *
 * Definition.  For a context of W x H output pixels, camera matrix `cam` and pixel (x, y) (row 0 = bottom, as everywhere): o = the
 * frame's ray origin (cam * (0,0,0,1)), d = the reference's primary direction of the pixel (src/update-cpu.cpp:82-89).  Run the
 * reference's nearest-hit loop (src/update-cpu.cpp:50-56): objects in index order, t = intersect_ray(object, o, d), accepted iff
 * t >= EPS (1e-7) && t < MAX_T (1e6) && t < best_t -- the lowest index wins a tie.  Then per pixel
 *     object  int32        index of the accepted object                                   miss: -1
 *     t       float64      best_t: ray parameter along the unit direction d, i.e. the distance from the eye      miss: +inf
 *     normal  4 x float32  (float) n.x, (float) n.y, (float) n.z, 0.0f with n = normal_vector(object, o + best_t * d)
 *                          (include/surface_impl.h:157-172: the normalised gradient, never flipped towards the eye), every component
 *                          rounded once from FP64, to nearest even                         miss: four +0.0f
 * Only the primary ray counts: a mirror shows itself, not what it reflects (rt_pick_paths and rt_trace_paths, "Ray queries", follow the
 * reflections).  Each plane is [local_rows][W] in the context's own row
 * layout (rt_local_rows, rt_row_map), so bands and ranks work as for the framebuffer; the planes do not depend on cfg.format.
 * Strict contexts compute exactly these values for surfaces of degree <= 2 (degree 3: as the render kernels, within their guard's
 * 1e-8 of t under the device's cbrt / acos / cos); RT_FLAG_FAST contexts run the FMA-contracted build of the same kernels.
 * (A unit sphere's normal comes from three of its coefficients; the terms left out are exact zeros, which can only change the sign
 * of a normal component that is itself an exact zero, and only for a hit point with a negative-zero coordinate.)
 *
 * Limits: primary hit only; contexts created with RT_FLAG_SSAA2, RT_FLAG_SSAA4 or RT_FLAG_SSAA_ADAPTIVE are refused (their frame
 * arguments describe another pixel grid; supporting them is a follow-up); the multi-GPU layer's entry point is
 * rt_render_gbuffer_multi ("Several GPUs"); a rank-level caller gathers the planes itself with rt_row_map and rt_assemble_planes.
 *
 * The pass reads the context's scene (constant between rt_set_scene calls) and camera-plane tables (constant after rt_create) and
 * nothing else: no tile words, launch-order generations, census, counters or frame tag.  Interleaving it with rt_render, on the same or another stream, changes no image and no
 * later G-buffer; it needs no ordering against the context's frames -- only against rt_set_scene, see "Scene updates".
 * ------------------------------------------------------------------------------------------------- */
typedef struct rt_hit {
    double t;         /* distance from the eye, +inf on a miss */
    double point[3];  /* o[i] + t * d[i] (multiply and add rounded separately in strict contexts); 0 on a miss */
    float normal[3];  /* as the normal plane; 0 on a miss */
    int32_t object;   /* -1 on a miss */
} rt_hit;             /* 48 bytes */

/* Enqueue one G-buffer pass for this rank's rows on `stream`.  Any of the three device pointers may be NULL (that plane is not
 * written), not all three.  ms as in rt_render: NULL = enqueue only (capturable into a graph), else synchronise and report the
 * device time of the pass.  RT_ERR_INVALID for a NULL context / camera, three NULL planes and supersampling contexts. */
int rt_render_gbuffer(rt_ctx *ctx, const double cam[16], int32_t *dev_object, double *dev_t, float *dev_normal, void *stream, float *ms);
/* n pixels by GLOBAL coordinates xy[2*i], xy[2*i+1] (any row, whatever this rank owns); blocks and writes n records to host memory.
 * Same per-ray function as the planes: a picked pixel is bit-equal to the planes' entry.  RT_ERR_INVALID for NULL arguments, n == 0,
 * a coordinate outside W x H (all n are checked before anything is enqueued) and supersampling contexts.  The staging buffers are the
 * context's own (allocated on the first call, freed by rt_destroy); calls on one context must not overlap in time. */
int rt_pick(rt_ctx *ctx, const double cam[16], const uint32_t *xy, uint32_t n, rt_hit *out_host, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Object extents: which objects a camera sees, where on the screen, how far away (csrc/rt_gbuffer.hip)
 *
 * Definition, in the G-buffer's terms: obj(x, y) and t(x, y) are the `object` and `t` entries of the G-buffer definition for this
 * context and `cam`; P is the set of pixels that lie in `rect` (x0, y0, x1, y1 inclusive, GLOBAL coordinates, row 0 = bottom; NULL = the
 * whole W x H frame) and in a row this rank owns.  Record i describes { (x, y) in P : obj(x, y) == i }: `pixels` is its size, the four
 * bounds are the minima and maxima of x and y over it, t_min / t_max the minimum and maximum of t(x, y) over it.  An object that owns
 * no pixel of P gets the identities of those reductions -- pixels = 0, x_min = y_min = 0xFFFFFFFF, x_max = y_max = 0, t_min = +inf,
 * t_max = +0.0 --, so the records of several ranks merge by sum / min / max without a special case.  Misses get no record: the caller
 * has |P| minus the sum of `pixels`.
 *
 * Accuracy is the G-buffer's: in every context kind rt_render_gbuffer accepts, the records are bit for bit the reduction of the planes
 * rt_render_gbuffer writes for the same context and camera (degree 3 and RT_FLAG_FAST included: the same per-ray function on the same
 * 16 x 16 tiles and 8 x 8 blocks); hence they equal the reference's nearest-hit loop for surfaces of degree <= 2 in strict contexts.
 * The result does not depend on the order of execution: every step is an integer sum, minimum or maximum (t is in [1e-7, 1e6), so the
 * bits of the double order as an unsigned integer).
 *
 * Like the G-buffer pass it reads the scene and the camera-plane tables and nothing else -- no tile words, census, counters (with
 * RT_FLAG_COUNT it books nothing) or frame tag --, needs no ordering against rt_render, and does need the caller's ordering against
 * rt_set_scene on another stream ("Scene updates").  Only the tiles that meet `rect` are traced.
 *
 * The multi-GPU layer's entry point is rt_object_extents_multi ("Several GPUs"); a rank-level caller merges the ranks' records with
 * rt_merge_object_extents.  Out of scope: supersampling contexts are refused as by rt_render_gbuffer; and only the primary hit counts: an object seen through a mirror is
 * not seen (a caller that wants it reduces the `dev_last` records of rt_trace_paths on the rays of rt_primary_rays itself).
 * ------------------------------------------------------------------------------------------------- */
typedef struct rt_object_extent {
    uint64_t pixels;                      /* pixels whose primary hit is this object */
    uint32_t x_min, y_min, x_max, y_max;  /* inclusive, GLOBAL pixel coordinates, row 0 = bottom */
    double   t_min, t_max;                /* smallest / largest best_t over those pixels */
} rt_object_extent;                       /* 40 bytes, 8-byte aligned */

/* Enqueue on `stream`: n_objects records into device memory (8-byte aligned).  ms as in rt_render_gbuffer: NULL = enqueue only, and the
 * call can be captured into a graph, to which it adds two kernel nodes (one that writes the identities, then the reduction; a rank
 * that owns no row of `rect` adds the first only and so still writes the identities); else synchronise and report the device time.  A
 * scene without objects returns RT_OK and enqueues nothing.  RT_ERR_INVALID for a NULL context / camera / output, an output that is
 * not 8-byte aligned, a `rect` with x0 > x1, y0 > y1, x1 >= W or y1 >= H, and supersampling contexts; RT_ERR_SCENE for a scene whose
 * class tables exceed the LDS of a workgroup, as rt_render_gbuffer (not with RT_FLAG_STREAM_QUERIES). */
int rt_object_extents(rt_ctx *ctx, const double cam[16], const uint32_t rect[4] /* x0,y0,x1,y1 inclusive, or NULL */,
                      rt_object_extent *dev_out /* [n_objects] */, void *stream, float *ms);
/* The same into host memory (any alignment: the records are copied there); blocks.  The staging buffer is the context's own (allocated on the first call, freed by rt_destroy); a
 * capturing stream is refused (RT_ERR_INVALID): the call allocates and waits. */
int rt_object_extents_host(rt_ctx *ctx, const double cam[16], const uint32_t rect[4],
                           rt_object_extent *out_host, void *stream);   /* blocks */
/* The records of several ranks into one: dev_parts = [n_parts][n_objects] records (n_objects = the context's); dev_out[i] = pixels summed,
 * x_min / y_min / t_min the minimum, x_max / y_max / t_max the maximum over the parts.  t is compared as the unsigned integer of its
 * bits, as the reduction kernel does.  All-identity in gives identity out, bit for bit.  Device pointers, one kernel on `stream`
 * (csrc/rt_planes.hip); a scene without objects returns RT_OK and enqueues nothing.  RT_ERR_INVALID, before a device is looked for:
 * NULL arguments, n_parts == 0, records not 8-byte aligned, an output that overlaps the parts. */
int rt_merge_object_extents(rt_ctx *ctx, const rt_object_extent *dev_parts, uint32_t n_parts, rt_object_extent *dev_out, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Ray queries: closest hit, occlusion and colour for rays the caller supplies (csrc/rt_rays.hip, csrc/rt_shade_rays.hip; DESIGN.md
 * sections 15 and 16)
 *
 * The G-buffer and rt_pick answer "what does the primary ray of this pixel hit"; these answer it for ANY ray: a reflection followed
 * from a hit point, a shadow ray towards a light, another camera (orthographic, fisheye, stereo, cube map), a line-of-sight or
 * collision probe.  A ray is an origin and a direction; the direction is used exactly as given, never normalised, so t is in units
 * of |d| as in intersect_ray (include/surface_impl.h:21).
 *
 * Closest hit.  The reference's nearest-hit loop (src/update-cpu.cpp:50-56) over the scene's objects in index order:
 * t = intersect_ray(object, o, d), accepted iff t >= EPS (1e-7) && t < MAX_T (1e6) && t < best_t -- the lowest index wins a tie.  One
 * rt_hit per ray: object; t = best_t; point[i] = o[i] + t * d[i] (multiply and add rounded separately in strict contexts);
 * normal = (float) normal_vector(object, point) (include/surface_impl.h:157-172), never flipped.  A miss gives object = -1, t = +inf
 * and +0.0 in point and normal: exactly what rt_pick writes.
 *
 * Occlusion.  The reference's shadow loop (src/update-cpu.cpp:66-72): ray i is blocked iff some object gives
 * t > EPS && t < t_max[i] -- both comparisons strict, and `>` where the closest hit has `>=`.  t_max is a device array of n doubles;
 * NULL means MAX_T (1e6) for every ray; a NaN t_max blocks nothing.  One int32 per ray, 1 (blocked) or 0.
 *
 * Nothing is skipped on the caller's behalf in either query: no own-sphere rule, no shadow bias, no round trip of the direction
 * through float.  A caller that wants the reference's shadow decision for a hit (point sp, normal n in FP64) and a light forms the
 * ray itself, as include/light_impl.h:17-27 and src/update-cpu.cpp:67 do:
 *     o = sp + SHADOW_BIAS * n          SHADOW_BIAS = 1e-2 (include/surface_impl.h:18)
 *     directional light:  d = (double) (float) light.p,         t_max = 1e6
 *     point light:        d = (double) (float) (light.p - sp),   t_max = 1.0       (the difference in FP64, then rounded to float)
 * and lights the hit where the ray is not blocked.  (rt_hit carries the normal in float; the reference's own decision uses the FP64
 * normal, which a caller recomputes from the surface's coefficients at `point` when it needs the reference's bits.)
 *
 * Accuracy.  Strict contexts compute exactly these values for surfaces of degree <= 2, for every ray: zero directions, |d|^2 <= EPS
 * (the reference's linear branch) and non-finite components included; a NaN t is never accepted.  The class tables and the deferred
 * root solves are used where they are proven -- every component of o and d at most 1e100 in magnitude, so that no monomial
 * overflows -- and every other ray goes through the reference's dense 20-term expansion, object by object.  Degree 3 behaves as the
 * render kernels do: the same guarded Taylor form with the dense fallback, within the guard's 1e-8 of t under the device's cbrt /
 * acos / cos.  RT_FLAG_FAST contexts run the FMA-contracted build of the same kernel; their results are their own arithmetic and are
 * not promised equal to rt_pick's (two kernels cannot promise that under contraction).
 *
 * Ray queries carry no frame state, so they work in EVERY context: plain, RT_FLAG_SSAA2 / RT_FLAG_SSAA4, adaptive, any rank or world,
 * any format.  They read the scene blob and nothing else -- no camera tables, tile words, launch-order generations, census, counters
 * or frame tag -- and need no ordering against rt_render (against rt_set_scene they do: "Scene updates").  Scenes whose class
 * tables exceed the LDS limit are refused as rt_render_gbuffer refuses them (not with RT_FLAG_STREAM_QUERIES).  With several GPUs they are called on rt_multi_query_ctx's context ("Several GPUs").
 *
 * Colour (rt_shade_rays; csrc/rt_shade_rays.hip).  The reference's render_pixel (src/update-cpu.cpp:82-119) with
 * ray_origin := o and dir := d, d used exactly as given, never normalised.  The first segment is get_color_and_object
 * (src/update-cpu.cpp:45-80): the closest hit above; sp = o + t * d; sn = normal_vector(sp) in FP64, never flipped; every light in index
 * order with shadow_ray (include/light_impl.h:17-27: the direction through float, max_t 1 or 1e6) from sp + SHADOW_BIAS * sn, blocked
 * iff some object gives t > EPS && t < max_t; the unblocked lights add surface_color (include/light_impl.h:29-44) in float32; each
 * component is clamped with (x < 1.0f) ? x : 1.0f.  Then the reflection loop of lines 96-117: reflection_ratio > EPS compared in double,
 * cur_ratio *= ratio in float, reflect_ray of the direction as it is, the new origin sp + SHADOW_BIAS * sn, UPDATE_COLOR as
 * (1.0f - r) * res + r * c; the scene's max_reflections cap and a bounce that leaves the scene both blend the background; a
 * first-segment miss is the background colour.  A scene without lights gives black hits, not the background.
 * Output is four float32 per ray, (r, g, b, 1.0f), whatever cfg.format is (as the G-buffer planes do not depend on the format): exactly
 * what an RT_FMT_RGBA32F pixel of rt_render holds when the ray is that pixel's primary ray.  dev_hits, when not NULL, receives the
 * rt_hit of the first segment, bit-equal to what rt_trace_rays writes for the same ray.
 * Accuracy as above: strict contexts compute exactly these values for surfaces of degree <= 2, for every ray -- zero directions,
 * non-finite components and components beyond 1e100 included -- and the FP32 colour operations are not contracted; degree 3 behaves as
 * the render kernels do; RT_FLAG_FAST contexts run the FMA-contracted build, whose colours are its own arithmetic.  Whether the class
 * tables are proven is decided for EVERY ray the kernel traces, not only the caller's: a hit at t < 1e6 along |d| <= 1e100 can put sp
 * beyond 1e100 and a vanishing gradient makes sn NaN, and the shadow and bounce rays derived from them then take the dense expansion.
 * None of the render kernels' work removal (facing-away skip, own-sphere rule, bounding-volume culling) is applied.
 * No frame state, as the other ray queries: every context kind, no ordering against rt_render, one kernel with ms == NULL (capturable
 * into a graph), and RT_FLAG_COUNT books none of its rays.
 * ------------------------------------------------------------------------------------------------- */
typedef struct rt_ray {
    double o[3]; /* origin */
    double d[3]; /* direction, used as given */
} rt_ray;        /* 48 bytes; 16-byte aligned in device memory */

/* n rays -> n rt_hit, both in device memory, on `stream`.  ms as in rt_render_gbuffer: NULL = enqueue only (one kernel, capturable
 * into a graph), else synchronise and report the device time of the pass.  RT_ERR_INVALID for a NULL context or pointer, n == 0, a
 * ray or hit pointer that is not 16-byte aligned, and input and output ranges that overlap. */
int rt_trace_rays(rt_ctx *ctx, const rt_ray *dev_rays, uint32_t n, rt_hit *dev_hits, void *stream, float *ms);
/* n rays (and n t_max values, or NULL) -> n int32 flags, all in device memory.  Refusals as rt_trace_rays (dev_t_max may be NULL; the
 * flags must overlap neither the rays nor t_max). */
int rt_occluded_rays(rt_ctx *ctx, const rt_ray *dev_rays, const double *dev_t_max, uint32_t n, int32_t *dev_blocked, void *stream, float *ms);
/* rt_trace_rays for rays and records in HOST memory; blocks.  The staging buffers are the context's own (they grow as rt_pick's do,
 * rt_destroy frees them); calls on one context must not overlap in time. */
int rt_trace_rays_host(rt_ctx *ctx, const rt_ray *rays, uint32_t n, rt_hit *out, void *stream);
/* n rays -> n pixels of 4 x float32 (r, g, b, 1.0f), optionally n rt_hit of the rays themselves (dev_hits may be NULL); all in device
 * memory, on `stream`; ms as in rt_trace_rays.  RT_ERR_INVALID for a NULL context, dev_rays or dev_rgba and for n == 0 (both before a
 * device is looked for), rays, rgba or hits that are not 16-byte aligned, and any overlap between input and output ranges or between
 * the two outputs.  Scenes beyond the LDS limit are refused as by rt_trace_rays (not with RT_FLAG_STREAM_QUERIES). */
int rt_shade_rays(rt_ctx *ctx, const rt_ray *dev_rays, uint32_t n, float *dev_rgba, rt_hit *dev_hits /* may be NULL */, void *stream, float *ms);
/* rt_shade_rays for rays and pixels in HOST memory; blocks.  Staging buffers as rt_trace_rays_host. */
int rt_shade_rays_host(rt_ctx *ctx, const rt_ray *rays, uint32_t n, float *rgba_out, void *stream); /* host memory, blocks */

/* Paths: the hits along a ray's mirror bounces (csrc/rt_paths.hip).
 *
 * A path is the geometry of the reference's render_pixel (src/update-cpu.cpp:82-119) with ray_origin := o and dir := d, as rt_shade_rays
 * defines it, minus everything that concerns colour.  R is the scene's max_reflections.
 *     (o_0, d_0) = (o, d);  ratio = 1.0f;  k = 0
 *     loop:
 *       h_k = closest hit of (o_k, d_k)            -- exactly rt_trace_rays' definition (t >= EPS, t < MAX_T, nearest, lowest index on a tie)
 *       miss:  end = (k == 0) ? RT_PATH_MISS : RT_PATH_ESCAPED;  segments = k;  stop
 *       sp = o_k + t * d_k  (FP64);   sn = normal_vector(object, sp)  (FP64, never flipped)
 *       if !((double) reflection_ratio[object] > EPS):   end = RT_PATH_SURFACE;  segments = k + 1;  stop      -- a NaN ratio is no mirror
 *       ratio = ratio * reflection_ratio[object]          (float32, one rounding)
 *       if k == R:                                        end = RT_PATH_CAP;      segments = k + 1;  stop
 *       d_{k+1} = reflect_ray(d_k, sn)   (include/light_impl.h:46-49, the direction as it is, never normalised)
 *       o_{k+1} = sp + SHADOW_BIAS * sn;   k = k + 1
 * The order of the ratio product and the cap test is the reference's (lines 101-107): a path that ends at the cap has the last mirror's
 * ratio in `ratio`.
 *
 * Outputs.  dev_segments is segment-major: record k * n + i is hit k of ray i as an rt_hit, its t, point and float normal those of
 * segment k, t in units of |d_k|; plane 0 is what rt_trace_rays writes for the same rays.  Every one of the max_segments planes is
 * written: a segment the path did not reach is the miss record (object -1, t +inf, zeros), so the caller never reads memory the call did
 * not define.  max_segments is a storage limit only: the path is followed to its end whatever it is, so dev_ends and dev_last do not
 * depend on it.  dev_last is the hit of segment `segments - 1`, the miss record when segments == 0; with `end` it answers "what does this
 * ray finally show": an object (RT_PATH_SURFACE) or the background (RT_PATH_MISS, RT_PATH_ESCAPED, RT_PATH_CAP).  The direction of an
 * escaped ray is not reported.  A mirror-aware form of rt_object_extents is a reduction of dev_last and is left to the caller.
 *
 * Accuracy is rt_shade_rays' (the same arithmetic without the lights): strict contexts are exact for surfaces of degree <= 2, for every
 * ray, non-finite components and components beyond 1e100 included.  Whether the class tables are proven is decided for every segment's
 * ray, not only the caller's: a derived ray can leave the proven range (a hit point beyond 1e100, a NaN normal where a gradient vanishes),
 * and such lanes go through the dense expansion.  Degree 3 behaves as the render kernels do.  RT_FLAG_FAST contexts run the
 * FMA-contracted build, whose results are their own arithmetic.
 * No frame state: paths work in every context kind, supersampling included, need no ordering against rt_render (against rt_set_scene on
 * another stream the ordering is the caller's, "Scene updates"), are one kernel with ms == NULL (capturable into a graph), and
 * RT_FLAG_COUNT books none of their rays.  With several GPUs: rt_multi_query_ctx's context. */
#define RT_PATH_MISS 0u     /* the ray itself hits nothing; segments = 0 */
#define RT_PATH_SURFACE 1u  /* the last hit is no mirror: that is what the ray finally shows */
#define RT_PATH_ESCAPED 2u  /* a bounce left the scene: the reference blends the background */
#define RT_PATH_CAP 3u      /* max_reflections bounces taken, the last hit is still a mirror: the reference blends the background */
#define RT_PATH_MAX_SEGMENTS 64u
typedef struct rt_path_end {
    uint32_t segments;  /* hits along the path, 0 .. max_reflections + 1 */
    uint32_t end;       /* RT_PATH_* */
    float    ratio;     /* cur_ratio as the reference's last UPDATE_COLOR used it; 1.0f when no mirror was met */
    int32_t  object;    /* object of the last hit, -1 when segments == 0 */
} rt_path_end;          /* 16 bytes, 16-byte aligned in device memory */

/* n rays -> max_segments planes of n rt_hit, optionally n rt_hit of the last hits, n rt_path_end; all in device memory, on `stream`; ms
 * as in rt_trace_rays.  RT_ERR_INVALID for a NULL context, dev_rays or dev_ends and for n == 0 (all before a device is looked for),
 * max_segments > RT_PATH_MAX_SEGMENTS, dev_segments == NULL with max_segments != 0 and the reverse, any pointer that is not 16-byte
 * aligned, and any overlap between the input range and an output range or between two output ranges.  Scenes beyond the LDS limit are
 * refused as by rt_trace_rays (not with RT_FLAG_STREAM_QUERIES). */
int rt_trace_paths(rt_ctx *ctx, const rt_ray *dev_rays, uint32_t n, uint32_t max_segments,
                   rt_hit *dev_segments /* [max_segments][n], or NULL iff max_segments == 0 */,
                   rt_hit *dev_last /* [n] or NULL */, rt_path_end *dev_ends /* [n] */, void *stream, float *ms);
/* rt_trace_paths for rays and records in HOST memory; blocks.  The staging buffer is the context's own (it grows as rt_pick's do,
 * rt_destroy frees it); calls on one context must not overlap in time. */
int rt_trace_paths_host(rt_ctx *ctx, const rt_ray *rays, uint32_t n, uint32_t max_segments,
                        rt_hit *segments_out, rt_hit *last_out /* may be NULL */, rt_path_end *ends_out, void *stream); /* blocks */

/* The context's own primary rays as explicit rays.  For every pixel (x, y) of `rect` (GLOBAL coordinates, whatever rows this rank owns,
 * as rt_pick) one rt_ray: o = the frame's ray origin (cam * (0,0,0,1)), d = the primary direction of the pixel, both bit for bit what the
 * render, G-buffer and pick kernels use (the same function on the context's camera-plane tables), hence the reference's
 * src/update-cpu.cpp:82-89.  The kernel reads the camera-plane tables and writes the rays, nothing else; with ms == NULL it is one
 * kernel and can be captured, so whole-frame colours, hits, occlusion and paths can be formed and traced in one graph without the host.
 * On a strict context without supersampling, with rays = rt_primary_rays(cam): rt_shade_rays(rays) is the RGBA32F frame of
 * rt_render(cam); for surfaces of degree <= 2 rt_trace_rays(rays) is rt_pick of those pixels (degree 3: the two form the cubic's data at
 * the origin differently, one on the host and one per lane, so only the ray queries' degree-3 accuracy is promised).
 * RT_ERR_INVALID for a NULL context / camera / output, an output that is not 16-byte aligned, a `rect` as rt_object_extents refuses it,
 * and supersampling contexts (refused as by rt_render_gbuffer: their tables describe another pixel grid). */
int rt_primary_rays(rt_ctx *ctx, const double cam[16], const uint32_t rect[4] /* x0,y0,x1,y1 inclusive, GLOBAL, or NULL = W x H */,
                    rt_ray *dev_rays /* [(y1-y0+1)][(x1-x0+1)], row y0 first, row 0 = bottom */, void *stream, float *ms);
/* Pick through mirrors: the primary rays of n pixels (GLOBAL coordinates xy[2*i], xy[2*i+1]; the list form of rt_primary_rays' kernel),
 * then rt_trace_paths, on the context's staging buffer; blocks and writes host memory.  Refusals, staging growth and the rule "calls
 * on one context must not overlap in time" are rt_pick's, plus rt_trace_paths' for max_segments.  For surfaces of degree <= 2 plane 0 is
 * rt_pick's record bit for bit; ends[i].object is what pixel i finally shows when ends[i].end == RT_PATH_SURFACE. */
int rt_pick_paths(rt_ctx *ctx, const double cam[16], const uint32_t *xy, uint32_t n, uint32_t max_segments,
                  rt_hit *segments_host /* [max_segments][n] or NULL iff 0 */, rt_path_end *ends_host, void *stream); /* blocks */

/* ---------------------------------------------------------------------------------------------------
 * Sorting rays: order caller-supplied rays on the device for culling (csrc/rt_sort_rays.hip)
 *
 * RT_FLAG_STREAM_CULL_RAYS culls per wave, and a wave is 64 consecutive rays of the caller's array: rays in an unrelated order make every
 * wave stage nearly every chunk (above: 98.5 % staged for the shuffled frame).  A caller cannot produce a good order itself -- it depends
 * on which chunk bounds a ray reaches -- so rt_sort_rays does, from the rays alone:
 *     rt_sort_rays(rays -> sorted, perm); rt_permute(perm, t_max -> t_max', gather); <any ray query on sorted>; rt_permute(perm, result ->
 *     result in the caller's order, scatter).
 * The two calls take no scene state (ctx selects the device, the grid bound and the error conventions, as in rt_assemble_planes; every
 * context kind), allocate nothing, read nothing back, and launch what n alone decides: with ms == NULL they only enqueue kernels and can
 * be captured into a graph that stays valid for other rays of the same count.  They change nothing about any other call; per-ray results
 * do not depend on a ray's neighbours, so the scattered result is bit for bit the result of the query on the caller's order.
 *
 * The key (csrc/rt_ray_sort_key.hpp is its definition; FP64, never contracted, the same in strict and RT_FLAG_FAST contexts):
 *   class 0 = a ray the culled kernels can cull for (the predicate of RT_FLAG_STREAM_CULL_RAYS: finite, every |component| <= 1e100,
 *   1e-7 < |d|^2 < inf), class 1 = every other ray: key 0x80000000, so those stand together at the end, in input order, and spoil at most
 *   one mixed wave.  Class 0: key = mo << 18 | md.  mo = the 12-bit Morton code of the origin in a 16^3 grid over the box of the class-0
 *   origins (q = clamp(floor((o - lo) / (hi - lo) * 16), 0, 15) per axis, 0 where hi == lo; -0.0 counts as +0.0); md = the 18-bit Morton
 *   code of the direction in a 512^2 grid over the octahedral map of d / (|dx| + |dy| + |dz|) (where n.z < 0: (u, v) = ((1 - |n.y|)
 *   sign(n.x), (1 - |n.x|) sign(n.y)), sign(0) = +1; q = clamp(floor((u / 2 + 1 / 2) * 512), 0, 511)).
 * perm[i] = the index in dev_rays of the ray at place i: a STABLE sort by that key (equal keys keep their input order), deterministic --
 * a radix sort whose only atomics are integer sums and the box's minima and maxima.  dev_sorted (may be NULL): sorted[i] = rays[perm[i]].
 * dev_keys (may be NULL): the key of sorted[i], non-decreasing.
 *
 * Limits.  The key helps rays that share origins or directions (a camera's, a lens model's, a light's, bounce rays of one surface); rays
 * with unrelated origins AND directions stay as they were (CPU proxy: 3 072 random probes aimed at random clusters, 0 of 240 (wave, chunk)
 * pairs left unstaged before and after).  n up to 2^32 - 1; work space about 16.5 bytes per ray (rt_sort_rays_work_bytes).
 *
 * RT_ERR_INVALID, before a device is looked for: a NULL ctx / dev_rays / dev_perm / dev_work / dev_src / dev_dst; n == 0; rays or sorted
 * rays that are not 16-byte aligned; perm, keys, src or dst that are not 4-byte aligned; work_bytes below rt_sort_rays_work_bytes(n); any
 * overlap among the rays, the sorted rays, perm, keys and the work space; for rt_permute elem_bytes of 0, not a multiple of 4 or above
 * 256, planes == 0, src or perm overlapping dst.
 *
 * Measured (one MI355X; the 1080p frame's own 2 073 600 primary rays, the four-flag context, strict; medians of five series of 31
 * synchronised calls, us; tools/sort_rays_bench.py, profiles/sort_rays.txt), rt_trace_rays:
 *   spheres  rays      unsorted   rt_sort_rays  sorted call  rt_permute  sum      sum / unsorted  staged [1]/[0]
 *   10 000   shuffled  25 043.6   279.4         3 725.1      51.4        4 056.0  0.162           0.985 -> 0.113
 *   10 000   row        4 160.3   224.2         3 701.7      37.0        3 962.8  0.953           0.120 -> 0.113
 *   10 000   8x8 block  3 793.1   224.1         3 706.9      37.1        3 968.1  1.046           0.111 -> 0.112
 *    1 685   shuffled   4 240.1   279.9         1 572.0      51.3        1 903.1  0.449           1.000 -> 0.290
 *    1 685   row        1 498.8   225.7         1 572.1      37.0        1 834.9  1.224           0.300 -> 0.289
 *       65   shuffled     189.5   280.1           190.8      51.0          521.9  2.754           0.500 -> 0.500
 * rt_occluded_rays and rt_trace_paths follow rt_trace_rays (shuffled 0.16 - 0.17 x at 10 000 spheres, 0.44 x at 1 685); rt_shade_rays
 * 42.4 -> 11.2 ms shuffled and 11.9 -> 10.6 ms in row order at 10 000 spheres.  So: sort rays that come in no spatial order; leave rays
 * alone that a camera produced in scan-line or block order unless the scene has thousands of spheres; never at two chunks, where the sort
 * costs more than the query.  The CPU proxy of DESIGN.md section 31 (a distance rule, not a measurement) had predicted 0.997 -> 0.199
 * staged for shuffled rays at 10 000 spheres on a 128 x 96 frame.
 * ------------------------------------------------------------------------------------------------- */
/* bytes of device work space rt_sort_rays needs for n rays (0 for n == 0); non-decreasing in n */
size_t rt_sort_rays_work_bytes(uint32_t n);
/* ms as in rt_trace_rays (NULL: enqueue only, capturable) */
int rt_sort_rays(rt_ctx *ctx, const rt_ray *dev_rays, uint32_t n, rt_ray *dev_sorted, uint32_t *dev_perm, uint32_t *dev_keys,
                 void *dev_work, size_t work_bytes, void *stream, float *ms);
/* planes x n records of elem_bytes each (plane stride n * elem_bytes; 16-byte vectors where elem_bytes % 16 == 0 and both pointers allow):
 *   scatter == 0: dst[p][i] = src[p][perm[i]]   (bring t_max into the sorted order)
 *   scatter != 0: dst[p][perm[i]] = src[p][i]   (bring hits, flags, colours, path records back into the caller's order)
 * perm must be a permutation of 0 .. n - 1 (rt_sort_rays' output): its entries are not checked. */
int rt_permute(rt_ctx *ctx, const uint32_t *dev_perm, uint32_t n, const void *dev_src, void *dev_dst, uint32_t elem_bytes,
               uint32_t planes, int scatter, void *stream, float *ms);

/* ---------------------------------------------------------------------------------------------------
 * Scene updates: move objects and lights of a live context (csrc/rt_set_scene.hip)
 *
 * rt_create uploads the scene once; rt_set_scene rewrites it in stream order, without a new context: one kernel of one workgroup reads
 * raw descriptor arrays from DEVICE memory -- the layout and meaning of the rt_scene_desc arrays of the same names -- and rebuilds the
 * scene blob and both light tables with the very functions rt_create packs them with (csrc/rt_scene_pack.hpp), so the device holds,
 * byte for byte, what a fresh rt_create of the new scene with the same rt_config would have uploaded (rt_debug_scene_blob shows it) --
 * in a context whose RT_FLAG_STREAM_CULL decision is true: what rt_create packs for the new scene under the context's order of the
 * unit-sphere table, which rt_set_scene never changes (chosen at rt_create; the one exception is rt_reorder_scene below, which chooses
 * it anew), and the bounds of its chunks (rt_debug_stream_bounds).
 * Any of the five pointers may be NULL = "keep what the context holds" (the kernel takes those raw values from its own records), not all
 * five.  n_objects, n_lights and every light's kind are fixed, and so are the background, field of view and max_reflections.
 *
 * The layout rule.  Everything the host chose at rt_create (kernel instantiation, table sizes and offsets, LDS sizes, culling, the lean
 * path) stays valid without the host seeing the data, because an update is ACCEPTED if and only if a fresh rt_create would derive
 *   - the same class table (unit sphere / other quadric / plane / degree 3) for every object, hence the same slot;
 *   - the same cullability for every object (a unit sphere with finite r^2 > 0, or not);
 *   - the same "some object has reflection_ratio > 1e-7" for the scene;
 *   - the same light-table flags for every light: its direction keeps |(float) p|^2 > 1e-7 or keeps failing it, and "this light's
 *     colour and every albedo of the scene are finite" keeps its truth value;
 *   - bit-identical 20 coefficients for every degree-3 object (their per-frame Taylor data is formed on the host: cubic surfaces are
 *     frozen in this version; their albedo and reflection may change within the rule).
 * Otherwise it is REJECTED and the kernel writes nothing to the scene: all or nothing.  Either way the kernel bumps a counter in a
 * small device block of the context: `applied`, or `rejected` together with the reason (RT_SCENE_REJECT_*) and the index of the
 * first offender -- objects come before lights, the lowest index first, and for one object the lowest reason code;
 * RT_SCENE_REJECT_MIRROR names the first object that became a mirror in a scene without one, or the first that stopped being one when
 * no mirror is left; RT_SCENE_REJECT_LIGHT names the light (a non-finite albedo shows as the first light with finite colour).
 *
 * Ordering.  rt_set_scene takes part in the context's frame order exactly as rt_render does: same stream as the previous call = enqueue
 * only (one kernel, nothing else: `(rt_set_scene, rt_render) x K` can be captured into one graph, and a replay reads the device arrays
 * again, so rewriting them between replays animates the scene); another stream first waits for the event recorded behind the previous
 * call; the event is not recorded while capturing, and after a captured call a call on another stream is refused (RT_ERR_INVALID).
 * The arrays must stay unchanged until the kernel has run.  The passes that READ the scene -- rt_render_gbuffer, rt_pick, rt_object_extents, rt_trace_rays,
 * rt_occluded_rays, rt_shade_rays, rt_trace_paths, rt_primary_rays, rt_pick_paths and their _host forms -- need no ordering against rt_render, but they DO need ordering against
 * rt_set_scene when issued on another stream, and that ordering is the caller's to establish (on one stream it is automatic).
 * Frame-to-frame state (launch order, census, tile words) survives an update: it affects speed only, never the image, exactly as under
 * a moving camera.  Works in every context kind.  The multi-GPU layer's entry point is rt_set_scene_multi ("Several GPUs").
 *
 * Re-sorting (RT_FLAG_STREAM_CULL_REORDER; csrc/rt_reorder_scene.hip).  rt_set_scene rebuilds every slot of the
 * unit-sphere table from the slot's object and never moves an entry, so in a culling context the chunks of spheres that mix lose their
 * locality.  rt_reorder_scene puts the table the device holds NOW into the order rt_create's packer would choose for it: the spheres
 * with a bounding radius first, by the 63-bit Morton key of their centres over the box of those centres, ties by object index; the
 * spheres without a radius behind them in object-index order; and it rebuilds the chunk bounds.  Afterwards rt_debug_scene_blob and
 * rt_debug_stream_bounds return, byte for byte, what a fresh rt_create of the scene the context currently holds would have uploaded.
 * Entries are moved as they are (rt_set_scene has re-packed them); nothing else in the blob moves.  The layout rule above keeps the
 * number of bounded spheres fixed, and they stand first before and after: a chunk is finite or infinite after a reorder exactly as
 * before it.  No result depends on the order, so frames and queries are bit for bit what they were -- only the work changes.
 * The calling rules are rt_set_scene's: the call takes part in the context's frame order with the same stream, event and capture rules;
 * it enqueues kernels only -- no allocation, no host read-back, no wait -- and every launch shape was decided at rt_create (by the numbers
 * of unit spheres and of objects), so `(rt_set_scene, rt_reorder_scene, rt_render) x K` can be captured once and replayed; ordering
 * against reading passes on other streams is the caller's.  How often to reorder is the caller's choice too: rt_set_scene itself never
 * does it.  A context whose decision is false (rt_get_stream_cull_reorder) enqueues nothing and returns RT_OK.
 * ------------------------------------------------------------------------------------------------- */
typedef struct rt_scene_update {
    const double *coefs;       /* [n_objects][RT_NCOEF]  or NULL */
    const float *reflection;   /* [n_objects]            or NULL */
    const float *albedo;       /* [n_objects][3]         or NULL */
    const double *light_p;     /* [n_lights][3]          or NULL */
    const float *light_color;  /* [n_lights][3]          or NULL */
} rt_scene_update;             /* 40 bytes */

#define RT_SCENE_REJECT_CLASS 1u  /* an object would move to another class table */
#define RT_SCENE_REJECT_BOUND 2u  /* a unit sphere would gain or lose its bounding radius (r^2 <= 0 or not finite) */
#define RT_SCENE_REJECT_MIRROR 3u /* the scene would gain its first mirror or lose its last */
#define RT_SCENE_REJECT_CUBIC 4u  /* a coefficient of a degree-3 object differs */
#define RT_SCENE_REJECT_LIGHT 5u  /* a light's table flags would change */

/* Device pointers; enqueues one kernel on `stream` and returns.  RT_ERR_INVALID for a NULL context or struct (both before a device is
 * looked for), five NULL arrays, a pointer not aligned to its type (8 bytes for coefs / light_p, 4 for the others) and a non-NULL
 * array of a kind the scene has none of (objects / lights).  Whether the update was applied is on the device: rt_set_scene_status. */
int rt_set_scene(rt_ctx *ctx, const rt_scene_update *dev, void *stream);
/* The same for arrays in HOST memory; blocks.  The staging buffer is the context's own (allocated on first use, freed by rt_destroy);
 * calls on one context must not overlap in time.  RT_ERR_SCENE when the kernel rejected the update: rt_last_error() then names the
 * reason and the index.  RT_ERR_INVALID on a capturing stream (the call allocates and waits: capture rt_set_scene instead). */
int rt_set_scene_host(rt_ctx *ctx, const rt_scene_update *host, void *stream);
/* Waits for the context's last call (on that call's stream; no other stream of the device is stalled), then: updates applied and
 * rejected since rt_create, and the reason / index of the most recent rejection (0 / 0 before the first).  Any output pointer may be
 * NULL.  RT_ERR_INVALID while that stream is capturing. */
int rt_set_scene_status(rt_ctx *ctx, uint64_t *applied, uint64_t *rejected, uint32_t *reason, uint32_t *index);
/* Re-sort the unit-sphere table into rt_create's order and rebuild the chunk bounds ("Re-sorting" above); enqueues kernels on `stream`
 * and returns.  RT_ERR_INVALID for a NULL context, decided before a device is looked for. */
int rt_reorder_scene(rt_ctx *ctx, void *stream);
/* *on = 1 where rt_reorder_scene re-sorts (RT_FLAG_STREAM_CULL_REORDER on a context whose rt_get_stream_cull is 1), else 0.
 * RT_ERR_INVALID for a NULL context or a NULL `on`, decided before a device is looked for. */
int rt_get_stream_cull_reorder(const rt_ctx *ctx, uint32_t *on);
/* Diagnostics: the scene as the device holds it -- the blob, then DevLight[n_lights], then LightK[n_lights] (csrc/rt_scene_dev.h).
 * *bytes receives the size; out may be NULL (size only), else cap must be at least that.  Waits as rt_set_scene_status does. */
int rt_debug_scene_blob(rt_ctx *ctx, void *out, size_t cap, size_t *bytes);
/* Diagnostics of RT_FLAG_STREAM_CULL: the chunk-bound table as the device holds it, one 64-byte UsEntry (csrc/rt_scene_dev.h) per
 * 64-entry chunk of the blob's unit-sphere table.  Calling conventions of rt_debug_scene_blob; 0 bytes where rt_get_stream_cull says 0. */
int rt_debug_stream_bounds(rt_ctx *ctx, void *out, size_t cap, size_t *bytes);
/* Diagnostics of RT_FLAG_STREAM_CULL_GROUPS: the group-bound table as the device holds it, one 64-byte UsEntry per 64 chunk bounds.
 * Calling conventions of rt_debug_scene_blob; 0 bytes where rt_get_stream_groups says 0. */
int rt_debug_stream_group_bounds(rt_ctx *ctx, void *out, size_t cap, size_t *bytes);
/* ... and the group verdicts of rt_render (rt_get_stream_groups), eight words of their own, cumulative since rt_create.  Waits as
 * rt_set_scene_status does.
 *   [0] primary group verdicts asked (one per wave and group bound)      [1] primary groups entered
 *   [2] shadow group verdicts asked, one per (wave, segment, light, group) where culling applied, up to the occlusion early-out
 *   [3] shadow groups entered
 *   [4] bounce queries' group verdicts, one per (wave, segment >= 1, group bound)      [5] bounce groups entered by the wave's union
 *   [6], [7] 0
 * The words exist only when MI355RT_STREAM_CULL_STATS=1 was in the environment at rt_create and the decision is true; otherwise the
 * kernel counts nothing and the call answers RT_ERR_INVALID.  RT_ERR_INVALID for a NULL argument, before a device is looked for. */
int rt_debug_stream_groups(rt_ctx *ctx, uint64_t out[8]);
/* The work words of RT_FLAG_STREAM_CULL's kernel, cumulative since rt_create; waits for the context's last call as rt_set_scene_status does.
 *   [0] primary chunk decisions (one per wave and chunk bound asked)      [1] primary chunks staged
 *   [2] shadow chunk decisions, one per (wave, segment, light, chunk) where culling applied      [3] shadow chunks staged
 *   [4] shadow entries decided (the entries of the staged chunks)         [5] shadow entries swept
 *   [6] shadow queries (wave, segment, light) that ran unculled           [7] 0
 * A wave whose rays are all decided stops asking (the occlusion early-out), so [2] counts every chunk only in scenes of at most 64
 * chunks.  The words exist only when MI355RT_STREAM_CULL_STATS=1 was in the environment at rt_create and the decision is true;
 * otherwise the kernel counts nothing and the call answers RT_ERR_INVALID. */
int rt_debug_stream_cull(rt_ctx *ctx, uint64_t out[8]);
/* ... and the work words of the culling halo and refine kernels (rt_get_stream_cull_adaptive), eight words of their own, cumulative
 * since rt_create; rt_debug_stream_cull's words stay the plain pass's alone.  Waits as rt_set_scene_status does.
 *   [0] primary chunk decisions (one per wave, pass of its item loop and chunk bound asked)      [1] primary chunks staged
 *   [2] shadow chunk decisions      [3] shadow chunks staged      [4] shadow entries decided      [5] shadow entries swept
 *   [6] shadow queries (wave, segment, light) that ran unculled
 *   [7] segment-0 queries that ran without a cone (a ray beyond 1e100 in the wave, or no lane in use: a wholly off-image halo wave)
 * The words exist only when MI355RT_STREAM_CULL_STATS=1 was in the environment at rt_create, the decision is true and the scene does not
 * hold both general quadrics and degree-3 objects (the counting kernel for that pair does not fit two waves per SIMD and is not built);
 * otherwise the kernel counts nothing and the call answers RT_ERR_INVALID.  RT_ERR_INVALID for a NULL argument, before a device is
 * looked for. */
int rt_debug_stream_cull_adaptive(rt_ctx *ctx, uint64_t out[8]);
/* ... and the work words of the bounce queries of rt_render (rt_get_stream_cull_bounce), eight words of their own, cumulative since
 * rt_create; rt_debug_stream_cull's words keep counting the primary and shadow work of the same kernel exactly as before.  Waits as
 * rt_set_scene_status does.
 *   [0] bounce chunk decisions: one per (wave, segment >= 1 with a lane in use, chunk bound asked)      [1] bounce chunks staged
 *   [2] (lane, chunk) pairs asked by lanes that can be culled for      [3] of [2], the pairs that reach
 *   [4] bounce queries in which no lane in use could be culled for      [5] - [7] 0
 * The words exist only when MI355RT_STREAM_CULL_STATS=1 was in the environment at rt_create and the decision is true; otherwise the
 * kernel counts nothing and the call answers RT_ERR_INVALID.  RT_ERR_INVALID for a NULL argument, before a device is looked for. */
int rt_debug_stream_cull_bounce(rt_ctx *ctx, uint64_t out[8]);
/* ... and the work words of the culled ray queries (rt_get_stream_cull_rays), eight words that rt_trace_rays, rt_occluded_rays,
 * rt_shade_rays, rt_trace_paths and the calls that go through them share, cumulative since rt_create.  Waits as rt_set_scene_status does.
 *   [0] chunk decisions: one per (wave, query with a lane in use, chunk looked at before an early-out)      [1] chunks staged
 *   [2] (lane, chunk) pairs asked by lanes that can be culled for      [3] of [2], the pairs that reach
 *   [4] queries in which no lane in use could be culled for      [5] - [7] 0
 * A query is one nearest-hit or occlusion query of a wave: one per wave for rt_trace_rays and rt_occluded_rays, one per segment and one
 * per segment and light for rt_shade_rays, one per segment for rt_trace_paths.  Only an occlusion query has an early-out.
 * The words exist only when MI355RT_STREAM_CULL_STATS=1 was in the environment at rt_create and the decision is true; otherwise the
 * kernels count nothing and the call answers RT_ERR_INVALID.  RT_ERR_INVALID for a NULL argument, before a device is looked for. */
int rt_debug_stream_cull_rays(rt_ctx *ctx, uint64_t out[8]);
/* ... and the work words of the culled pixel queries (rt_get_stream_cull_pixels), eight words that rt_render_gbuffer, rt_pick,
 * rt_object_extents and the calls that go through them share, cumulative since rt_create.  Waits as rt_set_scene_status does.
 *   [0] chunk decisions: one per (wave, nearest-hit call with a live pixel, chunk)      [1] chunks staged
 *   [2] entries asked inside staged chunks      [3] entries swept      [4] - [7] 0
 * A wave makes one call per 8 x 8 block of the planes, per block of each tile of an extents rectangle, per 64 picked pixels; a pick's
 * cone culls nothing, so there [1] == [0].
 * The words exist only when MI355RT_STREAM_CULL_STATS=1 was in the environment at rt_create and the decision is true; otherwise the
 * kernels count nothing and the call answers RT_ERR_INVALID.  RT_ERR_INVALID for a NULL argument, before a device is looked for. */
int rt_debug_stream_cull_pixels(rt_ctx *ctx, uint64_t out[8]);

/* Replaces cleanup_update (include/update.h:8). */
int rt_destroy(rt_ctx *ctx);

/* ---------------------------------------------------------------------------------------------------
 * Several GPUs of one node behind one call -- libmi355rt_multi.so (links librccl; libmi355rt.so itself does not).
 * The reference is single-GPU (src/update-cuda.cu:160-190); BASELINE.json's north star tiles the rows over the GPUs of a
 * node and gathers them on one.  One process: a context per (device, part) with the rows band-cyclic
 * over all n_devices * parts contexts, every device rendering part after part on its own stream, finished parts
 * travelling to devices[0] by ncclSend / ncclRecv over xGMI on a second stream while the next part renders, and
 * rt_assemble restoring row order there.  host/src/update-hip.cpp uses it when MI355RT_DEVICES names more than one
 * device, so update() (include/update.h:7) returns the whole frame whatever the number of GPUs.
 *   devices    HIP ordinals; devices[0] is the root that ends up with the frame.  All distinct: RCCL.  One ordinal repeated
 *              n times: the same choreography with device-to-device copies instead of RCCL (for a one-GPU box).
 *   parts      contexts per device (0 = 1): more parts = finer overlap of transfer and rendering
 *   flags      RT_FLAG_* of every context, plus RT_MULTI_SELF_EXCHANGE
 * rt_render_multi: root_full_fb = device pointer on devices[0] receiving [height][width] pixels, or NULL for the object's
 * own buffer (rt_multi_fb); enqueue-only unless ms is given (then: device time on the root from the start of its render
 * to the end of the reassembly, transfers included) -- except with RT_MULTI_SPARSE, see there.  rt_multi_stream() is the root
 * stream the frame is complete on; every write of a frame into the full frame is ordered after what the caller enqueued on it before.
 * ------------------------------------------------------------------------------------------------- */
#define RT_MULTI_SELF_EXCHANGE 0x10000u /* one device: send its rows to itself through RCCL instead of rendering in place
                                           (exercises the RCCL path on a one-GPU box) */
#define RT_MULTI_BANDWISE 0x20000u      /* rows travel band by band straight into their place in the full frame (one ncclSend / ncclRecv pair per band,
                                         * one strided copy per context on the root device): no rank-major receive slots, no rt_assemble pass */
#define RT_MULTI_SPARSE 0x40000u        /* only the 16x16 tiles that are not pure background travel to the root (sparse messages, see rt_pack_sparse), in
                                         * either format.  Every context renders with rt_render into its own buffer and packs it into a message whose
                                         * capacity is all of its tiles (no overflow is possible); the root copies each message's 16-byte header to the
                                         * host, and only the used prefix (header, id array, count x tile bytes) travels.  rt_render_multi therefore
                                         * BLOCKS the calling thread until every context's header of this frame has reached the host (a wait for the
                                         * renders and packs, not for the whole frame).  The root rebuilds the frame on rt_multi_stream(): incrementally
                                         * (stamps owned by the object) into the object's own buffer, with a full fill + scatter into a caller's buffer.
                                         * Not together with RT_MULTI_BANDWISE. */
typedef struct rt_multi rt_multi;
int rt_create_multi(rt_multi **out, const rt_scene_desc *scene, const int *devices, uint32_t n_devices, uint32_t band_rows, uint32_t parts,
                    uint32_t flags, uint32_t format);
int rt_render_multi(rt_multi *m, const double cam[16], void *root_full_fb, float *ms);
int rt_multi_wait(rt_multi *m);                       /* host waits until the last frame is complete on the root */
void *rt_multi_fb(rt_multi *m);                       /* the object's own full-frame buffer on devices[0] */
void *rt_multi_stream(rt_multi *m);                   /* hipStream_t on devices[0] */
int rt_multi_download(rt_multi *m, void *host_dst, size_t bytes);
int rt_multi_info(const rt_multi *m, uint32_t *n_contexts, uint32_t *transport /* 0 in place, 1 device copies, 2 RCCL */);
/* Bytes of the last frame: bytes_sent = what the contexts delivered to the root's reassembly (RT_MULTI_SPARSE: the sum of the used
 * message prefixes, counted from the headers; the dense transports: every context's rows), bytes_dense = what the dense transport
 * delivers (height x width pixels).  Either pointer may be NULL.  0 / 0 before the first frame. */
int rt_multi_last_transfer(const rt_multi *m, uint64_t *bytes_sent, uint64_t *bytes_dense);
/* rt_set_ssaa_threshold on every context of the object (RT_FLAG_SSAA_ADAPTIVE objects only). */
int rt_multi_set_ssaa_threshold(rt_multi *m, float tau);
/* rt_set_ssaa_geometry on every context of the object (RT_FLAG_SSAA_GEOMETRY objects only). */
int rt_multi_set_ssaa_geometry(rt_multi *m, float min_cos);
/* Scene updates, queries, G-buffer and extents with several GPUs (csrc/rt_multi.cpp; DESIGN.md section 21 has the stream and event
 * order of each call).  All of them refuse an object on which an earlier call failed with part of it enqueued, as rt_render_multi
 * does, and leave the calling thread on the device it came with.
 *
 * rt_set_scene_multi: rt_set_scene on every context.  The arrays are in HOST memory, with the meaning of rt_set_scene_host (NULL =
 * keep, not all five).  The call copies them into a pinned block the object owns and, on every device's RENDER stream, enqueues the
 * upload into that device's copy and rt_set_scene for each of its contexts; it does not wait for them -- only, before it overwrites
 * the pinned block and the device copies, for the previous call's uploads and kernels.  The update is therefore ordered with every
 * context's frames exactly as on a single context: frames enqueued before it show the old scene, frames after it the new one.  Whether
 * it was applied is on the devices: rt_multi_set_scene_status waits for every context's last call and returns context 0's numbers
 * (every context gives the same verdict: the layout rule depends on the scene alone; RT_ERR_DEVICE if they ever differ).  A call that
 * fails after the first context has been enqueued leaves the contexts with different scenes and the object failed. */
int rt_set_scene_multi(rt_multi *m, const rt_scene_update *host);
int rt_multi_set_scene_status(rt_multi *m, uint64_t *applied, uint64_t *rejected, uint32_t *reason, uint32_t *index);
/* rt_reorder_scene on every context, on its device's render stream and in frame order, as rt_set_scene_multi enqueues rt_set_scene:
 * behind an earlier rt_set_scene_multi, in front of later frames.  Enqueue-only.  Contexts whose decision is false enqueue nothing. */
int rt_reorder_scene_multi(rt_multi *m);
/* The root's context 0, borrowed until rt_multi_destroy, for the queries that depend neither on row ownership nor on frame state:
 * rt_pick, rt_pick_paths, rt_primary_rays, rt_trace_rays, rt_occluded_rays, rt_shade_rays, rt_trace_paths and their _host forms, all on
 * rt_multi_stream(m), where they are ordered behind rt_set_scene_multi on the root.  Nothing else may be called on it: frames, scene
 * updates, the G-buffer, extents, thresholds and its destruction are the object's business.  NULL for a NULL object. */
rt_ctx *rt_multi_query_ctx(rt_multi *m);
/* rt_render_gbuffer over all contexts: full [height][width] planes in device memory on devices[0]; any of the three pointers may be
 * NULL, not all three.  Each context runs rt_render_gbuffer for its rows on its render stream, the rows travel to the root as the dense
 * frame's rows do under the object's transport (RT_MULTI_BANDWISE and RT_MULTI_SPARSE objects use the plain dense choreography here), and
 * rt_assemble_planes rebuilds each requested plane on rt_multi_stream(m).  Enqueue-only unless ms is given: then the device time on the
 * root from the first G-buffer kernel to the last reassembly.  Row y of every plane is bit for bit the row rt_render_gbuffer writes on a
 * context of that rank, world and band size; in strict contexts and for surfaces of degree <= 2 the planes therefore equal a single
 * context's.  The contexts' own refusals pass through unchanged (supersampling, scenes beyond the LDS limit -- none of
 * the latter where RT_FLAG_STREAM_QUERIES was among rt_create_multi's flags: it reaches every context). */
int rt_render_gbuffer_multi(rt_multi *m, const double cam[16], int32_t *root_object, double *root_t, float *root_normal, float *ms);
/* rt_object_extents over all contexts: each writes its records, the world x n_objects records travel to the root by device copies and
 * rt_merge_object_extents merges them on rt_multi_stream(m) into root_dev_out (device memory on devices[0], 8-byte aligned).  ms as
 * above.  The result is the merge of the rank-level records, always, and equals a single context's records in strict contexts for
 * surfaces of degree <= 2.  The _host form writes host memory and blocks. */
int rt_object_extents_multi(rt_multi *m, const double cam[16], const uint32_t rect[4], rt_object_extent *root_dev_out, float *ms);
int rt_object_extents_multi_host(rt_multi *m, const double cam[16], const uint32_t rect[4], rt_object_extent *out_host);
int rt_multi_destroy(rt_multi *m);

#ifdef __cplusplus
}
#endif
#endif /* MI355RT_H */
