"""The shading loop of the streamed kernels and of rt_shade_rays (csrc/rt_stream_shade.hpp: shade_loop), host side:
the loop's text exists once, every kernel that shades a ray runs it under a policy of its own, and the helpers around it exist once.
So do the bodies of the kernels for caller-supplied rays (csrc/rt_ray_kernels.hpp): the staged, the streamed and the
culled kernel of each query run one body over a query object, and what was written out per family -- the ray loads, the grid rule, the
records, the path loop, the shading policy -- is in one file.
And so do the bodies of the pixel queries (csrc/rt_pixel_kernels.hpp): the staged and the streamed kernel of the
G-buffer / picking and of the object extents run one body over a pixel query object, and each table path has one object loop.
And so do the adaptive passes (csrc/rt_ray_list.hpp, csrc/rt_wave_ball.hpp, csrc/rt_adaptive.hip): the three ray-list
kernels take their items, their resolve and their launch ladder from one header, the two classifiers run one body, and the ball around
a wave's hit points is formed in one place.
One kernel is the stated exception: stream_cull_bounce_frame_kernel holds the loop's text itself, because through the shared loop its
strict <true, true> instantiation needs 258 registers and loses its second wave per SIMD (profiles/stream_shared_loop.txt)."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")
MARKER = "the reflection loop, src/update-cpu.cpp:96-117"
LOOP = "rt_stream_shade.hpp"
KEEPS_ITS_COPY = "rt_stream_cull_bounce.hip"
BODIES = "rt_ray_kernels.hpp"
PIXEL_BODIES = "rt_pixel_kernels.hpp"
RAY_LIST = "rt_ray_list.hpp"      # the three ray-list kernels' items, resolve and launch ladder
WAVE_BALL = "rt_wave_ball.hpp"    # the ball around a wave's hit points
# file -> (kernel or body, its policy): the sites that run the shared loop.  The three shade_rays kernels are one site: their body
SITES = {
    BODIES: ("rk_shade_rays", "RkShade<Query>"),
    "rt_stream.hip": ("stream_frame_kernel", "SqShade"),
    "rt_stream_adaptive.hip": ("ray_list_stream_kernel", "SqShade"),
    "rt_stream_cull.hip": ("stream_cull_frame_kernel", "ScShade"),
    "rt_stream_cull_adaptive.hip": ("ray_list_cull_kernel", "ScaShade"),
}
STREAMED = sorted(glob.glob(os.path.join(CSRC, "rt_stream*")) + [os.path.join(CSRC, n) for n in ("rt_shade_rays.hip", "rt_shade.hpp", "rt_rayquery.hpp", "rt_adaptive.hip", "rt_gbuffer.hip", BODIES, PIXEL_BODIES, RAY_LIST, WAVE_BALL)])
# One of the nine kernels for caller-supplied rays keeps the text of its body, as stream_cull_bounce_frame_kernel keeps the loop's:
# through rk_path_query path_query_stream_kernel took 4 to 5 % longer on every series measured (profiles/ray_kernel_bodies.txt)
PATHS_KEEPS_ITS_COPY = ("rt_stream_queries.hip", "path_query_stream_kernel")
# the four pixel kernels: file -> ({kernel: the body it runs}, the query object it builds)
PIXEL_KERNELS = {
    "rt_gbuffer.hip": ({"gbuffer_kernel": "pk_gbuffer", "extents_kernel": "pk_extents"}, r"RqPixels q = rq_stage_pixels<HAS_CUBIC>\(fa, scene, smem\);"),
    "rt_stream_queries.hip": ({"gbuffer_stream_kernel": "pk_gbuffer", "extents_stream_kernel": "pk_extents"}, r"SqPixels q\{fa, qa, scene, smem \+ \(threadIdx\.x >> 6\) \* SQ_SLICE_BYTES\};"),
}
# the other eight: file -> {kernel: the body it runs}
RAY_KERNELS = {
    "rt_rays.hip": {"ray_query_kernel": "rk_ray_query"}, "rt_shade_rays.hip": {"shade_rays_kernel": "rk_shade_rays"}, "rt_paths.hip": {"path_query_kernel": "rk_path_query"},
    "rt_stream_queries.hip": {"ray_query_stream_kernel": "rk_ray_query", "shade_rays_stream_kernel": "rk_shade_rays"},
    "rt_stream_cull_rays.hip": {"ray_query_cull_kernel": "rk_ray_query", "shade_rays_cull_kernel": "rk_shade_rays", "path_query_cull_kernel": "rk_path_query"},
}


def read(name):
    return open(os.path.join(CSRC, name)).read()


def code_of(name):
    return "\n".join(l.split("//")[0] for l in read(name).splitlines())


def test_the_loops_text_exists_once():
    """The marker comment of the reflection loop: in the shared loop, in the one body of the path kernels (rk_path_query: no lights, a
    store per segment -- another loop), and in the two kernels that keep a copy: stream_cull_bounce_frame_kernel the shared loop's,
    path_query_stream_kernel the path body's.  Nowhere else under csrc/."""
    have = {os.path.basename(p): open(p).read().count(MARKER) for p in glob.glob(os.path.join(CSRC, "*")) if MARKER in open(p).read()}
    assert have == {LOOP: 1, BODIES: 1, PATHS_KEEPS_ITS_COPY[0]: 1, KEEPS_ITS_COPY: 1}, have
    paths = read(BODIES).split("void rk_path_query(")[1].split("// ---- colour")[0]
    assert MARKER in paths
    assert MARKER in read(PATHS_KEEPS_ITS_COPY[0]).split(f"void {PATHS_KEEPS_ITS_COPY[1]}(")[1].split("// ---- pixels")[0]
    # what goes with the loop: the light loop's colour, the clamp and the blends are written in the same files only
    for word in ("surface_color(lt->p, lt->color, spherical, sp, sn, albedo)", "glm::min(vec3(1.0f), acc)", "RT_SYM(rtk)::blend(res, cur_ratio, bg)"):
        files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "rt_stream*")) + [os.path.join(CSRC, n) for n in ("rt_shade_rays.hip", BODIES)]
                       if word in open(p).read())
        assert files == sorted([LOOP, KEEPS_ITS_COPY]), (word, files)


def test_every_site_runs_the_shared_loop_under_its_own_policy():
    for name, (kernel, policy) in SITES.items():
        code = code_of(name)
        body = code.split(f"void {kernel}(")[1].split("\n}\n")[0]
        assert len(re.findall(r"shade_loop<HAS_GQ, HAS_CUBIC>\(", body)) == 1 and re.search(rf"\b{policy} pol{{", body), name
        assert code.count("shade_loop<") == 1, name
        assert "for (uint32_t k = 0; __ballot(bouncing) != 0ull; k++)" not in body, name
    # the one kernel outside: no call of the loop, its own bounce loop, and the two queries that make it what it is
    code = code_of(KEEPS_ITS_COPY)
    body = code.split("void stream_cull_bounce_frame_kernel(")[1].split("\n}\n")[0]
    assert "shade_loop" not in code and body.count("for (uint32_t k = 0; __ballot(bouncing) != 0ull; k++)") == 1
    assert "sc_query_primary<HAS_GQ, HAS_CUBIC>" in body and "sc_query_bounce<HAS_GQ, HAS_CUBIC>" in body


def test_the_copy_that_stays_is_the_loops_text():
    """stream_cull_bounce_frame_kernel's loop is shade_loop's, line for line, with the policy's hooks written in place: every line of the
    shared loop that calls no hook occurs in the kernel, in the same order."""
    def lines(text):
        return [l.strip() for l in text.splitlines() if l.strip()]
    loop = lines(code_of(LOOP).split("F3 shade_loop(")[1].split("\n    return res;\n")[0].split("bool bouncing = use;")[1])
    kernel = lines(code_of(KEEPS_ITS_COPY).split("void stream_cull_bounce_frame_kernel(")[1].split("bool bouncing = true;")[1].split("sc_flush(")[0].replace("fa.", "a."))
    shared = [l for l in loop if "pol." not in l]
    assert len([l for l in shared if len(l) > 12]) >= 35   # (most of them are expressions, not braces)
    assert len(shared) >= 45 and len(loop) - len(shared) == 4, (len(loop), len(shared))   # nearest, first_hit, segment, occluded
    at = 0
    for l in shared:
        assert l in kernel[at:], l
        at = kernel.index(l, at) + 1


def test_the_policies_state_the_four_points_and_nothing_workgroup_wide():
    header = read(LOOP)
    for word in ("All 64 lanes call", "`use` is a predicate", "no lane leaves before", "no barrier", "no hook puts divergent control flow around a staging call"):
        assert word.lower() in " ".join(header.lower().replace("//", " ").split()), word
    loop = code_of(LOOP).split("F3 shade_loop(")[1].split("struct ShadeNoSegment")[0]
    for hook in ("pol.template nearest<HAS_GQ, HAS_CUBIC>(k, lane, o, d, bouncing, best_t, best);", "if (k == 0u) pol.first_hit(best, best_t, sp, sn);",
                 "pol.segment(hit, sp);", "pol.template occluded<HAS_GQ, HAS_CUBIC>(seg, lane, *lt, so, sd, hit, max_t, blocked);"):
        assert loop.count(hook) == 1, hook
    assert loop.count("pol.") == 4
    # the per-segment hook sits behind the wave-uniform ballot, in front of the light loop
    assert re.search(r"if \(__ballot\(hit\) != 0ull\) \{\n[^\n]*albedo[^\n]*\n[^\n]*pol\.segment\(hit, sp\);\n\s*for \(uint32_t l = 0; l < a\.n_lights; l\+\+\)", loop)
    # (RkShade: the one policy of the three shade_rays kernels, a template over the query object)
    where = {"SqShade": LOOP, "ScShade": "rt_stream_cull.hpp", "ScaShade": "rt_stream_cull_adaptive.hip", "RkShade": BODIES}
    for policy, name in where.items():
        assert len(re.findall(rf"\bstruct {policy}\b[^;]*{{", code_of(name))) == 1, policy
        for other in set(where.values()) | {"rt_stream_shell.hpp", "rt_stream.hpp", "rt_stream_cull_bounce.hpp", "rt_shade_rays.hip", "rt_stream_queries.hip",
                                            "rt_stream_cull_rays.hpp", "rt_stream_cull_rays.hip", "rt_rayquery.hpp"}:
            if other != name:
                assert not re.search(rf"\bstruct {policy}\b", code_of(other)), (policy, other)
    assert "template <typename Query>\nstruct RkShade {" in code_of(BODIES)
    for p in glob.glob(os.path.join(CSRC, "*")):      # the three policies it replaces are gone
        for gone in ("ShadeRaysStaged", "SqkShadeRays", "ScRayShade"):
            assert gone not in open(p).read(), (gone, p)
    for name in (LOOP, "rt_stream_shell.hpp", RAY_LIST, BODIES):
        code = code_of(name)
        for word in ("__syncthreads", "s_barrier", '"workgroup"', "rq_stage_tables", "__shared__", "HIP_DYNAMIC_SHARED"):
            assert word not in code, (name, word)


def test_the_helpers_around_the_loop_exist_once():
    defs = {"quantise": r"uchar4 \w*quantise\(float x, float y, float z\)\s*{", "xor_add": r"F3 \w*xor_add\(const F3 &v, int m\)\s*{",
            "pixel mapping": r"tile_x \* 16u \+ \(wave & 1u\) \* 8u \+ \(lane & 7u\)", "frame store": r"\(res\.x \* 255\.0f \+ 0\.5f\)",
            "halo item": r"const int64_t gy = \(h & 1u\) \? g0 \+ rows : g0 - 1;", "resolve scale": r"constexpr float inv = 1\.0f / \(float\) \(K \* K\);"}
    found = {what: sorted(os.path.basename(p) for p in STREAMED for _ in re.findall(rx, "\n".join(l.split("//")[0] for l in open(p).read().splitlines())))
             for what, rx in defs.items()}
    assert found["quantise"] == ["rt_shade.hpp"] and found["xor_add"] == ["rt_shade.hpp"], found
    # (the pixel queries map pixels too -- once, for the staged and the streamed kernels and for both bodies: pk_block_pixel --, and so does the
    # one body of the two classify kernels of rt_adaptive.hip, classify_body: other kernels)
    assert found["pixel mapping"] == ["rt_adaptive.hip", PIXEL_BODIES, "rt_stream_shell.hpp"], found
    assert found["frame store"] == ["rt_stream_shell.hpp"], found
    # (ray_list_kernel, the twin over all records in LDS, takes its items and stores through the same header as the streamed twins)
    assert found["halo item"] == [RAY_LIST] and found["resolve scale"] == [RAY_LIST], found
    adaptive, ray_list = code_of("rt_adaptive.hip"), code_of(RAY_LIST)
    loop = adaptive.split("void ray_list_kernel(")[1].split("cnt.flush(counters);")[0].split("base += gridDim.x * WAVES * PPW) {")[1]
    assert [l.strip() for l in loop.splitlines() if l.strip()] == [
        "const SlItem it = sl_item<K>(fa, camx, camy, list, base + lane / LANES, n, i, j);", "if (it.use) cnt.primary();",
        "const F3 c = render_ray_culled<COUNT>(fa, gobj, glight, sobj, scull, origin, it.dir, it.use, cnt);", "sl_resolve_store<K, RGBA8>(fa, out, it, sub, c);", "}"], loop
    # the two classifiers run one body, which holds the walk, the ballot and the append; everything geometric sits behind its constant
    assert len(re.findall(r"void classify_body\(", adaptive)) == 1 and "template <bool RGBA8, bool GEOMETRY>\n__device__ __forceinline__ void classify_body(" in adaptive
    for kernel, call in (("classify_kernel", "classify_body<RGBA8, false>("), ("classify_geometry_kernel", "classify_body<RGBA8, true>(")):
        body = adaptive.split(f"void {kernel}(")[1].split("\n}\n")[0]
        assert body.count("classify_body<") == 1 and body.count(call) == 1 and "for (" not in body and "__ballot" not in body and "atomicAdd" not in body, kernel
    body = adaptive.split("void classify_body(")[1].split("\n}\n")[0]
    assert body.count("__ballot(") == 1 and body.count("atomicAdd(") == 1 and body.count("from_halo = ") == 3 and adaptive.count("from_halo = ") == 3
    plain = re.sub(r"\n( *)if constexpr \(GEOMETRY\) \{\n.*?\n\1\}\n", "\n", body, flags=re.S)      # the body without its two geometric blocks
    assert body.count("if constexpr (GEOMETRY) {") == 2 and "if constexpr" not in plain
    for word in ("obj[", "nrm[", "ghalo", "geo_dot", "min_cos)"):
        assert word in body and word not in plain.split("{", 1)[1], word
    # the ball around a wave's hit points is formed in one place (the wavefront kernel's own two sites apart)
    assert not re.search(r"\bwave_m(in|ax)\(double", adaptive) and "fmin(" not in adaptive and "fmax(" not in adaptive
    assert adaptive.count("wave_hit_ball<true>(hit, sp, ball)") == 1 and adaptive.count("wave_hit_ball") == 1 and "isfinite" not in adaptive
    everything = {os.path.basename(q): "\n".join(l.split("//")[0] for l in open(q).read().splitlines()) for q in glob.glob(os.path.join(CSRC, "*"))}
    assert {n: c.count("1.01e-2") for n, c in everything.items() if "1.01e-2" in c} == {"rt_wavefront.hip": 8, WAVE_BALL: 1}
    for fn in ("double wave_min(double", "double wave_max(double", "bool wave_hit_ball("):
        assert {n: c.count(fn) for n, c in everything.items() if fn in c} == {WAVE_BALL: 1}, fn
    ball = open(os.path.join(CSRC, WAVE_BALL)).read()
    assert "no colour and no RT_FLAG_COUNT counter depends on it" in ball
    # the (k, rgba8) ladder is written once, and all three launch files go through it
    assert sorted(n for n, c in everything.items() if "k == 4u" in c) == [RAY_LIST] and everything[RAY_LIST].count("k == 4u") == 1
    for name in ("rt_adaptive.hip", "rt_stream_adaptive.hip", "rt_stream_cull_adaptive.hip"):
        assert everything[name].count("return sl_for_shapes(k, rgba8, [&](auto kk, auto r8) {") == 1 and "#define" not in everything[name], name
    # the header has the standing of rt_stream_shell.hpp: nothing workgroup-wide, and no lane leaves sl_item early
    for name in (RAY_LIST, WAVE_BALL):
        for word in ("__syncthreads", "s_barrier", '"workgroup"', "rq_stage_tables", "__shared__", "HIP_DYNAMIC_SHARED"):
            assert word not in everything[name], (name, word)
    lists = ray_list.split("struct SlItem {")[1]
    assert lists.count("return") == 1 and "    return it;\n" in lists and "break" not in lists and "continue" not in lists
    assert '#include "rt_shade.hpp"' in ray_list and ray_list.count('#include "') == 1      # needs rt_shade.hpp alone
    # the work words leave through one function, and the class ladder of every launcher of these files is rq_for_classes
    assert len(re.findall(r"void sc_flush\(", code_of("rt_stream_cull.hpp"))) == 1
    for name in ("rt_stream_cull.hip", "rt_stream_cull_bounce.hip", "rt_stream_cull_adaptive.hip"):
        code = code_of(name)
        assert "sc_flush(st.w, ca.stats, lane" in code and "atomicAdd" not in code, name
    # (the ray kernels' files and the pixel family's two through the one macro over it, RK_LAUNCH, next to it in rt_rayquery.hpp)
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if "#define RK_LAUNCH" in open(p).read()) == ["rt_rayquery.hpp"]
    macro = read("rt_rayquery.hpp").split("#define RK_LAUNCH(fa, kernel, g, lds, stream, ...)")[1].split("\n\n")[0]
    assert "rq_for_classes(fa, [&](auto gq, auto cub) {" in macro and "hipLaunchKernelGGL(kernel, g, dim3(256), lds, stream, __VA_ARGS__);" in macro
    assert "#define" not in read("rt_stream_queries.hip") and "#define" not in read("rt_stream_cull_rays.hip")      # (no launch macro of their own)
    for name in list(SITES) + [KEEPS_ITS_COPY] + list(RAY_KERNELS) + list(PIXEL_KERNELS):
        code = code_of(name)
        if name in RAY_KERNELS or name in PIXEL_KERNELS:
            want = len(RAY_KERNELS.get(name, ())) + len(PIXEL_KERNELS.get(name, ((),))[0])
            assert len(re.findall(r"\bRK_LAUNCH\(fa, \(\w+<GQ, CUB[,>]", code)) >= want and "rq_for_classes" not in code, name
        elif name != BODIES:      # (the bodies' file launches nothing: the macro's text, held above, moved next to rq_for_classes)
            assert "rq_for_classes(fa, [&](auto gq, auto cub)" in code, name
        assert not re.search(r"kernel<(true|false), (true|false)", code) and "if (fa->n_cub)" not in code, name


def test_the_ray_kernels_bodies_exist_once():
    """each of the kernels (eight of the nine) takes its LDS, builds its query object and calls its body exactly
    once, with no loop of its own; the three-load ray read, the grid rule and the ray query's stores are written in one file, a path's
    stores in that file and in the one kernel that keeps the path body's text."""
    for name, kernels in RAY_KERNELS.items():
        code = code_of(name)
        for kernel, body_fn in kernels.items():
            body = code.split(f"void {kernel}(")[1].split("\n}\n")[0]
            assert len(re.findall(r"\brk_\w+<", body)) == 1 and len(re.findall(rf"\b{body_fn}<HAS_GQ, HAS_CUBIC(, OCCLUSION)?>\(", body)) == 1, (kernel, body)
            assert "for (" not in body and "while (" not in body and "shade_loop" not in body, kernel
            assert len(re.findall(r"\b(RqStaged|SqQuery|ScRayQuery) q\{", body)) == 1, kernel      # one query object, built here
        assert len(re.findall(r"\brk_(ray_query|shade_rays|path_query)<", code)) == len(kernels), name
    assert sum(len(k) for k in RAY_KERNELS.values()) == 8
    for body_fn in ("rk_ray_query", "rk_shade_rays", "rk_path_query"):
        assert len(re.findall(rf"void {body_fn}\(", code_of(BODIES))) == 1, body_fn
    # a query object offers one call
    for struct, name in (("RqStaged", "rt_rayquery.hpp"), ("SqQuery", "rt_stream.hpp"), ("ScRayQuery", "rt_stream_cull_rays.hpp")):
        text = code_of(name).split(f"struct {struct} {{")[1].split("\n};\n")[0]
        assert text.count("__device__") == 1 and "void query(uint32_t" in text and "template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION>" in text, struct
    everything = {os.path.basename(p): "\n".join(l.split("//")[0] for l in open(p).read().splitlines()) for p in glob.glob(os.path.join(CSRC, "*"))}
    only_in_bodies = ("const double2 w0 = w[0], w1 = w[1], w2 = w[2];",                       # the three-load ray read
                      "need < max_grid ? need : (max_grid ? max_grid : 1u)",                  # the grid rule
                      "out_blocked[i] = best;", "nv = normal_vector(gobj[best].c, p);", "RkShade<Query> pol{")
    for word in only_in_bodies:
        assert sorted(n for n, code in everything.items() if word in code) == [BODIES], word
    for word in ("rq_store_record(out_seg +", "out_end[i] = PathEnd{segments, end, cur_ratio, last};"):      # a path's stores
        assert sorted(n for n, code in everything.items() if word in code) == sorted([BODIES, PATHS_KEEPS_ITS_COPY[0]]), word
        assert everything[PATHS_KEEPS_ITS_COPY[0]].count(word) == everything[BODIES].count(word), word
    assert everything[BODIES].count("const double2 w0 = w[0], w1 = w[1], w2 = w[2];") == 1 and everything[BODIES].count("need < max_grid ?") == 1


def test_the_pixel_kernels_bodies_exist_once():
    """each of the four pixel kernels takes its LDS, builds its query object and calls its body exactly once, with no
    loop of its own but the accumulator init and flush of extents_kernel; a pixel query object offers one call; the record assembly, the
    sphere-normal special case, the block-cone formation, the extents wave reduction and the extents init kernel are written once under
    csrc/; what the copies were called is gone."""
    for name, (kernels, query) in PIXEL_KERNELS.items():
        code = code_of(name)
        for kernel, body_fn in kernels.items():
            body = code.split(f"void {kernel}(")[1].split("\n}\n")[0]
            assert len(re.findall(r"\bpk_\w+<", body)) == 1 and len(re.findall(rf"\b{body_fn}<HAS_GQ, HAS_CUBIC>\(", body)) == 1, (kernel, body)
            assert len(re.findall(query, body)) == 1 and len(re.findall(r"\b(RqPixels|SqPixels) q\b", body)) == 1, kernel      # one query object, built here
            loops = re.findall(r"for \([^\n]*", body)
            assert "while (" not in body and "nearest" not in body and "rq_tables" not in body and "sq_tables" not in body, kernel
            if kernel == "extents_kernel":      # the accumulators' identities and their flush, each with a barrier between it and the body
                assert len(loops) == 2 and all(l.startswith("for (uint32_t i = threadIdx.x; i < fa.n_obj; i += 256u)") for l in loops), loops
                at = [body.index(w) for w in ("rq_stage_pixels<", "acc[i] = ext_identity();", "__syncthreads();", "pk_extents<", "__syncthreads();\n        for (", "ext_merge<__HIP_MEMORY_SCOPE_AGENT>")]
                assert at == sorted(at) and len(set(at)) == 6 and body.count("__syncthreads()") == 2, at
            else:
                assert not loops and "__syncthreads" not in body, kernel
        assert len(re.findall(r"\bpk_(gbuffer|extents)<", code)) == len(kernels), name
    bodies = code_of(PIXEL_BODIES)
    for body_fn in ("pk_gbuffer", "pk_extents", "pk_block_pixel"):
        assert len(re.findall(rf"\b{body_fn}\(const FrameArgs &fa", bodies)) == 1, body_fn
    assert bodies.count("q.template nearest<HAS_GQ, HAS_CUBIC>(lane, m, ") == 2 and bodies.count("q.") == 2 and bodies.count("pk_block_pixel(fa, ") == 2
    # a pixel query object offers one call, and each lives next to the loop it calls
    for struct, name, loop in (("RqPixels", "rt_rayquery.hpp", "rq_tables<HAS_GQ, HAS_CUBIC, false, true>("), ("SqPixels", "rt_stream.hpp", "sq_tables<HAS_GQ, HAS_CUBIC, false, true>(")):
        text = code_of(name).split(f"struct {struct} {{")[1].split("\n};\n")[0]
        assert text.count("__device__") == 1 and "template <bool HAS_GQ, bool HAS_CUBIC>\n" in text, struct
        assert "void nearest(uint32_t lane, const Mono &m, bool live, bool block, double &best_t, int &best) const" in text and text.count(loop) == 1, struct
        assert "sq_pixel_cone(" in text and "rq_plain" not in text and "sq_query" not in text, struct
        assert sorted(n for n in os.listdir(CSRC) if re.search(rf"\bstruct {struct}\b", code_of(n))) == [name], struct
    # one object loop per table path: the staged one takes the cone and the host's records behind a switch that is off for everyone else
    staged = code_of("rt_rayquery.hpp")
    assert len(re.findall(r"void rq_tables\(", staged)) == 1 and "template <bool HAS_GQ, bool HAS_CUBIC, bool OCCLUSION, bool PRIMARY = false>\n__device__ __forceinline__ void rq_tables(" in staged
    assert staged.count("if (PRIMARY && cone.on) {") == 1 and staged.count("if (PRIMARY && j < RT_CUB_AT_MAX) {") == 1 and staged.count("PRIMARY") == 3
    assert len(re.findall(r"void sq_tables\(", code_of("rt_stream.hpp"))) == 1
    everything = {n: code_of(n) for n in os.listdir(CSRC)}
    users = {n: c.count("rq_tables<") for n, c in everything.items() if "rq_tables<" in c}
    assert users == {"rt_rayquery.hpp": 2}, users      # RqStaged::query, without the switch, and RqPixels::nearest
    assert "rq_tables<HAS_GQ, HAS_CUBIC, OCCLUSION>(qa, S, gobj, m, use && proven, t_max, best_t, best);" in staged
    once = {"r.n[0] = (float) n.x; r.n[1] = (float) n.y; r.n[2] = (float) n.z;": PIXEL_BODIES,                      # the record assembly
            "n = sphere_normal(e, p);": PIXEL_BODIES, "if (bo->cls & RT_CLS_UNITSQ) {": PIXEL_BODIES,                  # the sphere-normal special case
            "out_rec[blockIdx.x * 256u + tid] = r;": PIXEL_BODIES, "out_normal[at] = make_float4(": PIXEL_BODIES,      # the stores
            "sq_readlane(ca, 0), c1 = sq_readlane(ca, 7), c2 = sq_readlane(ca, 56), c3 = sq_readlane(ca, 63);": "rt_rayquery.hpp",      # the block-cone formation
            "if (cone.on && block) cone = sq_block_cone(d);": "rt_rayquery.hpp", "SqCone sq_block_cone(": "rt_rayquery.hpp", "double sq_readlane(": "rt_rayquery.hpp",
            "Mono rq_mono(": "rt_rayquery.hpp",                                                                        # the Mono set-up (below)
            "void ext_reduce_wave(": "rt_extents.hpp", "const unsigned long long l2 = __shfl_xor(lo, s), h2 = __shfl_xor(hi, s);": "rt_extents.hpp",      # the wave reduction
            "ExtRecord{0ull, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, RT_EXT_INF_BITS, 0ull}": "rt_extents.hpp",               # the identity, and the init kernel
            "void name(ExtRecord *__restrict__ out, uint32_t n)": "rt_extents.hpp",
            "(&fa.cub_rec[0][0])[threadIdx.x]": "rt_rayquery.hpp"}                                                       # the host's records behind the staged tables
    for word, where in once.items():
        assert sorted(n for n, c in everything.items() if word in c) == [where] and everything[where].count(word) == 1, word
    for n in ("rt_rayquery.hpp", "rt_stream.hpp", "rt_gbuffer.hip", "rt_stream_queries.hip", BODIES, PIXEL_BODIES):      # (the frame kernels' own set-ups: not this family's)
        assert everything[n].count("mono_set_od<NEED_CROSS>(m);") == (n == "rt_rayquery.hpp"), n
    assert sorted(n for n, c in everything.items() if "EXT_INIT_KERNEL(" in c) == ["rt_extents.hpp", "rt_gbuffer.hip", "rt_stream_queries.hip"]
    assert "EXT_INIT_KERNEL(extents_init_kernel)" in everything["rt_gbuffer.hip"] and "EXT_INIT_KERNEL(extents_init_stream_kernel)" in everything["rt_stream_queries.hip"]
    assert sum(c.count("extents_init") for c in everything.values()) == 4      # (each file: the definition and its launch)
    # the header has the standing of rt_ray_kernels.hpp: nothing workgroup-wide
    for word in ("__syncthreads", "s_barrier", '"workgroup"', "rq_stage_tables", "rq_stage_pixels", "__shared__", "HIP_DYNAMIC_SHARED"):
        assert word not in bodies, word
    for gone in ("GbRecord", "GbHit", "GbTables", "gb_readlane", "sqk_mono", "sqk_nearest_hit", "nearest_hit", "primary_hit", "rt_launch_gbuffer_edges", "gbuffer_edges"):
        for n in os.listdir(CSRC):
            assert gone not in read(n), (gone, n)
    # the G pass of an adaptive frame with the geometric term: the two launchers rt_render_gbuffer / rt_pick call, chosen by the context's one decision
    capi = code_of("rt_capi.cpp")
    g = capi.split("if (ctx->geometry) {")[1].split("RT_HIP(rt_launch_classify_geometry_strict(")[0]
    # (the streamed or the staged path of the launcher table -- DESIGN.md section 35 --, named here and never the pixel entry points' culled one)
    assert "const QueryLaunchers &g = ctx->kern->query[ctx->stream_adaptive ? PATH_STREAMED : PATH_STAGED];" in g
    assert "g.gbuffer(&fa, ctx->d_obj, ctx->d_camx, ctx->d_camy, ctx->d_geo_obj, nullptr, nrm, nullptr, stream)" in g
    assert "g.pick(&fa, ctx->d_obj, ctx->d_camx, ctx->d_camy, ctx->d_geo_xy, ctx->halo_slots * ctx->width, ctx->d_geo_halo, nullptr, stream)" in g
    assert g.count("RT_HIP(") == 2


def test_the_path_kernel_that_keeps_its_copy_is_the_bodys_text():
    """path_query_stream_kernel is rk_path_query line for line -- code and order -- from the grid-stride loop to its end, with the query
    object's one call written in place as sq_query without a cone; in front of the loop it takes its wave's slice as its twins do."""
    def lines(text):
        return [l.strip() for l in text.splitlines() if l.strip()]
    body = lines(code_of(BODIES).split("void rk_path_query(")[1].split("template <typename Query>")[0].split("const uint64_t stride =")[1])
    kernel = lines(code_of(PATHS_KEEPS_ITS_COPY[0]).split(f"void {PATHS_KEEPS_ITS_COPY[1]}(")[1].split("\n}\n")[0].split("const uint64_t stride =")[1])
    call = "q.template query<HAS_GQ, HAS_CUBIC, false>(lane, o, d, bouncing, MAX_T, best_t, best);"
    assert body.count(call) == 1 and len(body) >= 55
    want = [("sq_query<HAS_GQ, HAS_CUBIC, false>(qa, scene, slice, lane, o, d, bouncing, false, MAX_T, best_t, best);" if l == call else l) for l in body]
    assert kernel + ["}"] == want, [(a, b) for a, b in zip(kernel, want) if a != b][:3]      # (the body's text ends with its closing brace)
    head = code_of(PATHS_KEEPS_ITS_COPY[0]).split(f"void {PATHS_KEEPS_ITS_COPY[1]}(")[1].split("const uint64_t stride =")[0]
    for l in ("__shared__ __align__(16) unsigned char smem[4u * SQ_SLICE_BYTES];", "const RayQueryArgs &qa = pa.qa;", "const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;",
              "unsigned char *slice = smem + wave * SQ_SLICE_BYTES;", "const DevObject *gobj = reinterpret_cast<const DevObject *>(scene);"):
        assert l in head, l
    assert "rk_" not in head.replace("rk_load_ray", "")
