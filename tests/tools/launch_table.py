"""The launcher tables of the host side, read from the source text: what csrc/rt_launch.h declares and which slot of struct Kernels
(csrc/rt_capi.cpp, RT_KERNELS) holds which launcher.  The host tests of the single features ask it where their launcher went;
tests/test_launch_paths_host.py holds the whole table to the naming rule."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "cuda-ray-tracer_amd", "csrc")
QUERIES = ("gbuffer", "pick", "object_extents", "trace_rays", "occluded_rays", "shade_rays", "trace_paths")
PATHS = ("PATH_STAGED", "PATH_STREAMED", "PATH_CULLED")
VARIANTS = ("strict", "fast")


def read(name):
    return open(os.path.join(CSRC, name)).read()


def declared():
    """{launcher: its argument list} for every RT_PER_VARIANT(hipError_t, rt_launch_..., ...) of rt_launch.h, an argument macro (RT_..._ARGS)
    written out.  A launcher declared twice is an error."""
    text = read("rt_launch.h")
    joined = re.sub(r"\\\n", " ", text)
    macros = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"^#define (RT_\w+_ARGS)\s+(.*)$", joined, re.M)}
    out = {}
    for m in re.finditer(r"^RT_PER_VARIANT\(hipError_t, (rt_launch_\w+),\s*([^;{}]*?)\)\n", text, re.M):
        name, args = m.group(1), " ".join(m.group(2).split())
        assert name not in out, name
        out[name] = macros.get(args, args)
    return out


def slots():
    """{slot: launcher} of the one initialiser of struct Kernels, e.g. "query[PATH_CULLED].pick" -> "rt_launch_pixel_cull_pick".  Every
    statement of the initialiser must be `k.<slot> = RT_CAT(<launcher>, V);` -- nothing is filled by position --, no slot is named twice, and
    both instances (kernels_strict, kernels_fast) come from it."""
    capi = read("rt_capi.cpp")
    assert capi.count("#define RT_KERNELS(V)") == 1
    body = capi.split("#define RT_KERNELS(V)")[1].split("}()\n")[0]
    lines = [l.rstrip("\\").strip() for l in body.splitlines()]
    lines = [l for l in lines if l]
    assert lines[0] == "[] {" and lines[1] == "Kernels k{};" and lines[-1] == "return k;", (lines[:2], lines[-1])
    out = {}
    for l in lines[2:-1]:
        m = re.fullmatch(r"k\.([\w\[\]\.]+) = RT_CAT\((rt_launch_\w+), V\);", l)
        assert m, l
        assert m.group(1) not in out, l
        out[m.group(1)] = m.group(2)
    assert "static const Kernels kernels_strict = RT_KERNELS(strict), kernels_fast = RT_KERNELS(fast);" in capi
    assert len(re.findall(r"\bKernels\s+\w+\s*(=\s*)?\{[^}]", capi)) == 0 and capi.count("RT_KERNELS(") == 3      # no other instance, none by a brace list
    return out


def members():
    """The members of struct QueryLaunchers and of struct Kernels (rt_launch.h), as {member: launcher whose type it has}; `query` maps to
    "QueryLaunchers[3]"."""
    text = read("rt_launch.h")
    def of(struct):
        body = re.search(rf"struct {struct} \{{(.*?)\n\}};", text, flags=re.S).group(1)
        code = "\n".join(l.split("//")[0] for l in body.splitlines())
        out = {m.group(2): m.group(1) for m in re.finditer(r"decltype\(&(rt_launch_\w+)_strict\) (\w+);", code)}
        rest = re.sub(r"decltype\(&rt_launch_\w+_strict\) \w+;", "", code).split()
        return out, rest
    q, rest = of("QueryLaunchers")
    assert not rest, rest
    k, rest = of("Kernels")
    assert rest == ["QueryLaunchers", "query[3];"], rest
    k["query"] = "QueryLaunchers[3]"
    return q, k


def slot_of(launcher):
    """The one slot that names the launcher."""
    hits = [s for s, l in slots().items() if l == launcher]
    assert len(hits) == 1, (launcher, hits)
    return hits[0]
