"""The launcher table of the host side, from the source text: struct Kernels holds the seven query launchers once per
table path, every slot is filled by its name with the launcher of its own path and query, and no launcher is in two slots.  Every path of a
query returns the same bits, so a launcher in the wrong slot passes every parity test: this file and tests/test_launch_paths_gpu.py are
what would see it.  No GPU."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import launch_table as LT  # noqa: E402

PIXEL_QUERIES = ("gbuffer", "pick", "object_extents")
# the launcher of a path and a query: rt_launch_<prefix><query>; the culled pixel launchers are pixel_cull_*, the culled ray launchers stream_cull_*
PREFIX = {"PATH_STAGED": lambda q: "", "PATH_STREAMED": lambda q: "stream_", "PATH_CULLED": lambda q: "pixel_cull_" if q in PIXEL_QUERIES else "stream_cull_"}
# where each path's launchers are defined
FILES = {"PATH_STAGED": {"gbuffer": "rt_gbuffer.hip", "pick": "rt_gbuffer.hip", "object_extents": "rt_gbuffer.hip", "trace_rays": "rt_rays.hip",
                         "occluded_rays": "rt_rays.hip", "shade_rays": "rt_shade_rays.hip", "trace_paths": "rt_paths.hip"},
         "PATH_STREAMED": {q: "rt_stream_queries.hip" for q in LT.QUERIES},
         "PATH_CULLED": {q: "rt_stream_cull_pixels.hip" if q in PIXEL_QUERIES else "rt_stream_cull_rays.hip" for q in LT.QUERIES}}
# the launchers outside the table: their signatures differ by more than the chunks, so they stay members of their own
LOOSE = {"trace": "rt_launch_trace", "wavefront": "rt_launch_wavefront", "stream": "rt_launch_stream", "stream_cull": "rt_launch_stream_cull",
         "stream_cull_bounce": "rt_launch_stream_cull_bounce", "ray_list": "rt_launch_ray_list", "stream_ray_list": "rt_launch_stream_ray_list",
         "stream_cull_ray_list": "rt_launch_stream_cull_ray_list", "primary_rays": "rt_launch_primary_rays"}


def launcher(path, query):
    return f"rt_launch_{PREFIX[path](query)}{query}"


def test_the_header_has_one_record_one_enum_and_one_member_per_query():
    text = LT.read("rt_launch.h")
    assert re.search(r"struct ChunkTables \{\s*const void \*bounds;\s*uint32_t n_chunks;\s*unsigned long long \*stats;\s*\};", text)
    assert "enum TablePath { PATH_STAGED, PATH_STREAMED, PATH_CULLED };" in text
    query, kernels = LT.members()
    assert tuple(query) == LT.QUERIES and all(query[q] == f"rt_launch_{q}" for q in LT.QUERIES)      # one member per query, of the staged launcher's type
    assert kernels == dict(LOOSE, query="QueryLaunchers[3]")
    assert "The staged and the streamed launchers ignore `chunks`." in text


def test_every_slot_names_the_launcher_of_its_own_path_and_query():
    slots = LT.slots()      # (itself: one initialiser, every statement `k.<slot> = RT_CAT(<launcher>, V);`, no slot twice, both instances from it)
    want = {f"query[{p}].{q}": launcher(p, q) for p in LT.PATHS for q in LT.QUERIES}
    want.update(LOOSE)
    assert slots == want      # every slot filled, with its own launcher, and nothing else
    names = [f"{l}_{v}" for l in slots.values() for v in LT.VARIANTS]
    assert len(set(names)) == len(names) == 2 * (21 + len(LOOSE))
    table = [f"{launcher(p, q)}_{v}" for p in LT.PATHS for q in LT.QUERIES for v in LT.VARIANTS]
    assert len(set(table)) == 42


def test_one_signature_per_query_and_one_definition_per_launcher(pkg):
    decl = LT.declared()
    hips = {n: LT.read(n) for n in sorted(os.listdir(LT.CSRC)) if n.endswith(".hip")}
    makefile = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "Makefile")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for q in LT.QUERIES:
        args = {decl[launcher(p, q)] for p in LT.PATHS}
        assert len(args) == 1, q      # the three paths' launchers have one signature ...
        assert args.pop().endswith(", const ChunkTables *chunks, hipStream_t stream"), q      # ... the staged arguments, the chunks, the stream
        for p in LT.PATHS:
            name = launcher(p, q)
            where = [n for n, text in hips.items() if f"RT_SYM({name})(" in text]
            assert where == [FILES[p][q]] and hips[where[0]].count(f"RT_SYM({name})(") == 1, (name, where)
            assert re.search(rf"\$\(eval \$\(call VARIANT_RULES,{where[0][:-4]},", makefile), where      # (compiled once per variant)
            for v in LT.VARIANTS:
                assert re.search(rf"\bT {name}_{v}\b", exported), (name, v)
    # the frame, bounce and ray-list launchers that cull take the same record
    for name in ("rt_launch_stream_cull", "rt_launch_stream_cull_bounce", "rt_launch_stream_cull_ray_list"):
        assert "const ChunkTables *chunks" in decl[name] and "n_chunks" not in decl[name], name
    assert decl["rt_launch_stream_cull_bounce"].endswith("const ChunkTables *chunks, unsigned long long *bounce_stats, hipStream_t stream")


def test_the_call_sites_go_through_the_decision_and_the_old_ladders_are_gone():
    everything = "".join(LT.read(n) for n in os.listdir(LT.CSRC))
    for gone in ("RT_QUERY_KERNEL", "RT_CULL_RAYS_ARGS", "RT_CULL_PIXELS_ARGS"):
        assert gone not in everything, gone
    capi = LT.read("rt_capi.cpp")
    assert not re.search(r"ctx->stream_cull\w* \? ctx->kern->", capi) and "ctx->stream_cull" not in capi
    # the table is reached through the two decisions and, for the G pass, a path named on the spot: nowhere else
    uses = re.findall(r"kern->query\[[^;]*\];", capi)
    uses = [u[:-1] for u in uses]
    assert sorted(uses) == sorted(["kern->query[cull[CULL_PIXELS] ? PATH_CULLED : plain]", "kern->query[cull[CULL_RAYS] ? PATH_CULLED : plain]",
                                   "kern->query[ctx->stream_adaptive ? PATH_STREAMED : PATH_STAGED]"]), uses
    # ... and one rule says whether bounds belong to a scene's table
    rule = "chunks->n_chunks != (fa->n_us + SQ_CHUNK - 1u) / SQ_CHUNK"
    assert everything.count(rule) == 1 and rule in LT.read("rt_stream_cull.hpp") and "SQ_CHUNK - 1u) / SQ_CHUNK" not in everything.replace(rule, "")
    calls = {n: LT.read(n).count("sc_cull_args(fa, chunks, ca)") for n in os.listdir(LT.CSRC)}
    assert {n: c for n, c in calls.items() if c} == {"rt_stream_cull.hip": 1, "rt_stream_cull_bounce.hip": 1, "rt_stream_cull_adaptive.hip": 1, "rt_stream_cull_rays.hip": 3,
                                                     "rt_stream_cull_pixels.hip": 2}
    assert LT.read("rt_stream_cull_pixels.hip").count("fa->cull == 0u || !sc_cull_args(") == 2      # the pixel launchers' own condition: no cone, no culling
    assert "!sc_cull_args(fa, chunks, ca) || (ca.stats == nullptr) != (bounce_stats == nullptr)" in LT.read("rt_stream_cull_bounce.hip")


@pytest.mark.parametrize("family", ["", "_adaptive", "_bounce", "_rays", "_pixels"])
def test_the_family_entry_points_are_wrappers_over_two_helpers(pkg, family):
    capi = LT.read("rt_capi.cpp")
    enum = {"": "CULL_FRAME", "_adaptive": "CULL_ADAPTIVE", "_bounce": "CULL_BOUNCE", "_rays": "CULL_RAYS", "_pixels": "CULL_PIXELS"}[family]
    assert f'extern "C" int rt_get_stream_cull{family}(const rt_ctx *ctx, uint32_t *on) {{ return get_cull({enum}, ctx, on); }}' in capi
    assert f'extern "C" int rt_debug_stream_cull{family}(rt_ctx *ctx, uint64_t out[8]) {{ return debug_cull({enum}, ctx, out); }}' in capi
    order = re.search(r"enum CullFamily \{(.*?)\};", capi, flags=re.S).group(1)
    rows = re.search(r"cull_family\[N_CULL_FAMILIES\] = \{(.*?)\n\};", capi, flags=re.S).group(1)
    names = re.findall(r'\{"(rt_get_stream_cull\w*)", "(rt_debug_stream_cull\w*)",', rows)
    assert [n for n in re.findall(r"\b(CULL_\w+|N_CULL_FAMILIES)\b", "\n".join(l.split("//")[0] for l in order.splitlines()))][-1] == "N_CULL_FAMILIES"
    index = re.findall(r"\bCULL_\w+\b", "\n".join(l.split("//")[0] for l in order.splitlines())).index(enum)
    assert names[index] == (f"rt_get_stream_cull{family}", f"rt_debug_stream_cull{family}") and len(names) == 5      # the family's row is its enum value's
    # the refusals need no device, and say what they said
    import ctypes as C
    lib = pkg.lib()
    n, words = C.c_uint32(7), (C.c_uint64 * 8)(*([9] * 8))
    get, debug = getattr(lib, f"rt_get_stream_cull{family}"), getattr(lib, f"rt_debug_stream_cull{family}")
    assert get(None, C.byref(n)) == -1 and lib.rt_last_error() == f"rt_get_stream_cull{family}: null argument".encode() and n.value == 7
    assert get(C.c_void_p(16), None) == -1 and lib.rt_last_error() == f"rt_get_stream_cull{family}: null argument".encode()
    assert debug(None, words) == -1 and lib.rt_last_error() == f"rt_debug_stream_cull{family}: null argument".encode() and list(words) == [9] * 8
