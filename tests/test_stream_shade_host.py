"""The shading loop of the streamed kernels and of rt_shade_rays (csrc/rt_stream_shade.hpp: shade_loop), host side:
the loop's text exists once, every kernel that shades a ray runs it under a policy of its own, and the helpers around it exist once.
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
# file -> (kernel, its policy): the sites that run the shared loop
SITES = {
    "rt_shade_rays.hip": ("shade_rays_kernel", "ShadeRaysStaged"),
    "rt_stream_queries.hip": ("shade_rays_stream_kernel", "SqkShadeRays"),
    "rt_stream.hip": ("stream_frame_kernel", "SqShade"),
    "rt_stream_adaptive.hip": ("ray_list_stream_kernel", "SqShade"),
    "rt_stream_cull.hip": ("stream_cull_frame_kernel", "ScShade"),
    "rt_stream_cull_adaptive.hip": ("ray_list_cull_kernel", "ScaShade"),
}
STREAMED = sorted(glob.glob(os.path.join(CSRC, "rt_stream*")) + [os.path.join(CSRC, n) for n in ("rt_shade_rays.hip", "rt_shade.hpp", "rt_rayquery.hpp", "rt_adaptive.hip")])


def read(name):
    return open(os.path.join(CSRC, name)).read()


def code_of(name):
    return "\n".join(l.split("//")[0] for l in read(name).splitlines())


def test_the_loops_text_exists_once():
    """The marker comment of the reflection loop: in the shared loop, in the two path kernels (rt_paths.hip, and once in
    rt_stream_queries.hip for path_query_stream_kernel: no lights, a store per segment -- another loop), and in the one kernel that keeps
    its copy.  Nowhere else under csrc/."""
    have = {os.path.basename(p): open(p).read().count(MARKER) for p in glob.glob(os.path.join(CSRC, "*")) if MARKER in open(p).read()}
    assert have == {LOOP: 1, "rt_paths.hip": 1, "rt_stream_queries.hip": 1, KEEPS_ITS_COPY: 1}, have
    paths = read("rt_stream_queries.hip").split("void path_query_stream_kernel")[1].split("// ---- pixels")[0]
    assert MARKER in paths
    # what goes with the loop: the light loop's colour, the clamp and the blends are written in the same files only
    for word in ("surface_color(lt->p, lt->color, spherical, sp, sn, albedo)", "glm::min(vec3(1.0f), acc)", "RT_SYM(rtk)::blend(res, cur_ratio, bg)"):
        files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "rt_stream*")) + [os.path.join(CSRC, "rt_shade_rays.hip")] if word in open(p).read())
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
    where = {"SqShade": LOOP, "ScShade": "rt_stream_cull.hpp", "ScaShade": "rt_stream_cull_adaptive.hip", "ShadeRaysStaged": "rt_shade_rays.hip",
             "SqkShadeRays": "rt_stream_queries.hip"}
    for policy, name in where.items():
        assert len(re.findall(rf"\bstruct {policy}\b[^;]*{{", code_of(name))) == 1, policy
        for other in set(where.values()) | {"rt_stream_shell.hpp", "rt_stream.hpp", "rt_stream_cull_bounce.hpp"}:
            if other != name:
                assert not re.search(rf"\bstruct {policy}\b", code_of(other)), (policy, other)
    for name in (LOOP, "rt_stream_shell.hpp"):
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
    # (gbuffer_stream_kernel maps pixels too, with picking beside it, and so do the two classify kernels of rt_adaptive.hip: other kernels)
    assert found["pixel mapping"] == ["rt_adaptive.hip", "rt_adaptive.hip", "rt_stream_queries.hip", "rt_stream_shell.hpp"], found
    assert found["frame store"] == ["rt_stream_shell.hpp"], found
    # (ray_list_kernel, the twin over all records in LDS, keeps its own items: it counts, and skips by `live`)
    assert found["halo item"] == ["rt_adaptive.hip", "rt_stream_shell.hpp"] and found["resolve scale"] == ["rt_adaptive.hip", "rt_stream_shell.hpp"], found
    # the work words leave through one function, and the class ladder of every launcher of these files is rq_for_classes
    assert len(re.findall(r"void sc_flush\(", code_of("rt_stream_cull.hpp"))) == 1
    for name in ("rt_stream_cull.hip", "rt_stream_cull_bounce.hip", "rt_stream_cull_adaptive.hip"):
        code = code_of(name)
        assert "sc_flush(st.w, ca.stats, lane" in code and "atomicAdd" not in code, name
    for name in list(SITES) + [KEEPS_ITS_COPY]:
        code = code_of(name)
        assert "rq_for_classes(fa, [&](auto gq, auto cub)" in code and not re.search(r"kernel<(true|false), (true|false)", code), name
