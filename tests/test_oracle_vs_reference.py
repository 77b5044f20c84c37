"""The CPU oracle (oracle/rt_oracle.c, the restatement) held to a build of the reference's own CPU path, bit for bit.

oracle/Makefile.ref compiles the reference's update-cpu.cpp, surface.cpp, light.cpp, scene-exception.cpp, surface_impl.h and
light_impl.h unmodified into oracle/_ref/ (tests/tools/ref_binary.py runs them).  Every GPU test, smoke() and bench.py's CPU legs
trust the oracle on shipped, random and edge scenes; this module checks it there against the text it restates: whole frames through
the reference's init_update / update, and its functions one call at a time.

Every comparison is on the raw bits (ref_binary.same_bits: a NaN only has to be a NaN on both sides).  There is no tolerance in
this module: both sides are IEEE double / float arithmetic without contraction on one host, and both call the same glibc.

What this does not pin: the operation order of glm is the stand-in's (oracle/ref_shim/), the reference's YAML
loader is not built, and both sides share the host's glibc and compiler (the -O0 build against the -O2 build is the evidence that
the optimiser does not matter)."""
import functools
import importlib.util
import os
import sys

import ctypes as C
import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ref_binary as R  # noqa: E402

SCENES = ["quadratic", "20spheres", "reflection_test", "clebsch", "cayley", "cubic", "dingdong", "monkey_saddle"]
SIZES = [(96, 72), (53, 31), (40, 64), (1, 1)]   # two non-square sizes the other way round, an odd one, one pixel
EPS, MAX_T = 1e-7, 1e6                           # surface_impl.h:16,19
N = 3000                                         # inputs per class of a per-function batch


@pytest.fixture(scope="module", autouse=True)
def ref_programs():
    return R.require()


def bits_equal(got, want, what):
    assert R.same_bits(got, want), f"{what}: {mismatches(got, want)} values differ from the reference"


def mismatches(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return f"shape {a.shape} against {b.shape};"
    with np.errstate(invalid="ignore"):
        return int(((a != b) & ~(np.isnan(a) & np.isnan(b))).sum())


# ---- cameras -----------------------------------------------------------------------------------------------------------------
def behind_first_surface(O, sc):
    """A camera position just past the first crossing of some object's surface, seen from the origin: inside a closed object, on
    the far side of an open one."""
    fan = [(x, y, 1.0) for y in (0.0, -0.3, 0.3, -0.6, 0.6, -2.0, -8.0) for x in (0.0, -0.3, 0.3, -0.6, 0.6)]
    for obj in sc.objects:
        c = (C.c_double * 20)(*obj.c)
        for d in fan:
            t = O.lib().orc_intersect_ray(c, O._d3((0, 0, 0)), O._d3(d))
            if 0.5 <= t < 1000.0:
                return tuple((t + 0.05) * v for v in d)
    raise AssertionError("nothing in front of the origin")


def cameras(O, sc):
    roll = np.eye(4)   # a general matrix: camera_matrix() never rolls -- 30 degrees about the view axis, then moved
    roll[0, 0], roll[0, 1], roll[1, 0], roll[1, 1] = np.cos(0.5), -np.sin(0.5), np.sin(0.5), np.cos(0.5)
    roll[:3, 3] = (-0.4, 0.3, -1.0)
    return {
        "identity": None,
        "start_up": O.camera_matrix(),                                   # src/ray-tracer.cpp: position 0, yaw 90, pitch 0
        "moved": O.camera_matrix((0.3, 0.2, -0.5), 80.0, 10.0),
        "golden_moved": O.camera_matrix((0.7, 0.9, -2.5), 84.0, 6.0),    # tests/tools/make_golden.py
        "rolled": roll.T.reshape(16).copy(),                             # column-major
        "inside": O.camera_matrix(behind_first_surface(O, sc), 90.0, 0.0),
        "away": O.camera_matrix((0.0, 0.0, -2.0), 270.0, 35.0),          # looks along -z and up: the scenes are at +z
    }


# ---- 1. frames of the shipped scenes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_shipped_scene_frames(oracle, name, size):
    """Every shipped scene, seven cameras, four sizes: update() of the reference, its surfaces and lights built by the reference's
    own factories from the scene file's arguments, against Scene.render() of the oracle."""
    w, h = size
    sc = oracle.load_scene(scene_path(name)).with_size(w, h, 3)
    cams = cameras(oracle, sc)
    ref = R.RefScene.from_yaml(scene_path(name)).render(list(cams.values()), w, h, 3)
    for i, (cname, cam) in enumerate(cams.items()):
        want = sc.render(cam=cam, nthreads=4)
        bits_equal(want, ref[i], f"{name} {w}x{h} camera {cname}")
        if (w, h) == (96, 72) and cname in ("identity", "start_up", "moved"):
            assert int((want != sc.bg_color).any(-1).sum()) >= 200, f"{name}: camera {cname} sees nothing"
    if name == "20spheres":
        assert np.all(ref[list(cams).index("away")] == sc.bg_color), "the camera that looks away sees an object"


@pytest.mark.parametrize("name", SCENES)
def test_reflection_depths(oracle, name):
    """max_reflections 0 .. 5 and 7 (past the loader's default of 5)."""
    cams = [None, oracle.camera_matrix((0.3, 0.2, -0.5), 80.0, 10.0)]
    ref_scene = R.RefScene.from_yaml(scene_path(name))
    frames = []
    for depth in (0, 1, 2, 3, 4, 5, 7):
        sc = oracle.load_scene(scene_path(name)).with_size(64, 48, depth)
        want = np.stack([sc.render(cam=cam) for cam in cams])
        bits_equal(want, ref_scene.render(cams, 64, 48, depth), f"{name} depth {depth}")
        frames.append(want)
    if any(o.reflection_ratio > EPS for o in sc.objects):
        assert not np.array_equal(frames[0], frames[1]), f"{name} has a mirror, and the depth limit changes nothing"


@pytest.mark.parametrize("name", ["20spheres", "reflection_test", "clebsch", "monkey_saddle", "quadratic"])
def test_unoptimised_build_renders_the_same_frames(oracle, name):
    """The same reference sources at -O0 and at -O2: what is pinned does not hang on the host compiler's optimiser."""
    sc = oracle.load_scene(scene_path(name)).with_size(64, 48, 3)
    cams = [None, oracle.camera_matrix((0.3, 0.2, -0.5), 80.0, 10.0)]
    o2, o0 = R.render(sc, cams, opt="O2"), R.render(sc, cams, opt="O0")
    assert R.same_bits(o0, o2), f"{name}: {mismatches(o0, o2)} values differ between the -O0 and the -O2 build of the reference"


def test_golden_frames_are_the_references(oracle):
    """tests/golden/frames_96x72.npz was rendered by the oracle (tests/tools/make_golden.py): all 8 scenes at 96x72 with the
    loader's max_reflections, identity and moved camera.  The reference renders the same 16 frames."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "frames_96x72.npz"))
    frames = [k for k in g.files if not k.startswith("cam_")]
    assert len(frames) == 16
    for key in frames:
        name, cname = key.split("__")
        ref = R.RefScene.from_yaml(scene_path(name)).render([g["cam_" + cname]], 96, 72)[0]
        bits_equal(g[key], ref, f"golden frame {key}")


# ---- 2. the random and edge scenes the GPU suites trust the oracle on --------------------------------------------------------
def _tool(name):
    """tests/tools/<name>.py as a module.  fuzz_spheres sets MI355RT_LEAN for its own command-line runs when it is imported; a test
    process must not keep that."""
    keep = os.environ.get("MI355RT_LEAN")
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        if keep is None:
            os.environ.pop("MI355RT_LEAN", None)
        else:
            os.environ["MI355RT_LEAN"] = keep


_tool = functools.lru_cache(maxsize=None)(_tool)


def built_scene(pkg, oracle, key):
    """key -> (oracle scene, camera), through the builders of the GPU suites (imported, not copied)."""
    from test_gpu_parity import oracle_from, random_cubic_scene
    kind = key[0]
    if kind in ("fuzz_spheres", "fuzz_parity", "fuzz_cubic"):
        s, cam = _tool(kind).scene(key[1])[:2]
    elif kind == "random_cubic":
        s, cam = random_cubic_scene(pkg, key[1], 96, 72)
    else:
        from test_counters_fuzz_gpu import build   # ("random", ...), ("mixed", ...), ("edge", name), ("shear", seed)
        _, osc, cam = build(key)
        return osc, cam
    return oracle_from(pkg, oracle, s), cam


def _built_keys():
    from test_counters_fuzz_gpu import RANDOM, SHEAR
    from test_ssaa_adaptive_fuzz_gpu import EDGE
    keys = [("fuzz_spheres", s) for s in range(14)]
    keys += [("fuzz_parity", s) for s in [158, 534] + list(range(2000, 2024))]
    keys += [("fuzz_cubic", s) for s in range(8)] + [("random_cubic", s) for s in range(6)]
    keys += [("mixed", s, 96, 72) for s in range(12)]
    keys += RANDOM + SHEAR                           # sphere fields up to 200 objects and 40 lights; general (sheared) camera matrices
    keys += [("edge", n) for n in EDGE]              # no objects, no lights, 1x1, own-sphere corners, offsets up to 3e7, two mirrors, ...
    return keys


@pytest.mark.parametrize("key", _built_keys(), ids=lambda k: "-".join(str(v) for v in k[:3]))
def test_random_and_edge_scenes_of_the_gpu_suites(pkg, oracle, key):
    """The inputs on which the GPU tests take the oracle's word: the sphere fields of fuzz_spheres, the mixed classes of fuzz_parity,
    the random cubics of fuzz_cubic and test_gpu_parity, the random fields / mixed scenes / sheared cameras / edge scenes of
    test_counters_fuzz_gpu and test_ssaa_adaptive_fuzz_gpu."""
    osc, cam = built_scene(pkg, oracle, key)
    bits_equal(osc.render(cam=cam, nthreads=4), R.render(osc, [cam])[0], str(key))


def _raw():
    return _tool("raw_desc_scenes")


def _raw_names():
    import raw_desc_scenes as S
    return list(S.NAMED)


def _raw_seeds():
    import raw_desc_scenes as S
    return list(range(S.N_SEEDS))


@pytest.mark.parametrize("name", _raw_names())
def test_raw_descriptor_named_scenes(oracle, name):
    """tests/tools/raw_desc_scenes.py: directional lights of any length (short, zero, long, NaN, inf), colours, albedos, reflection
    ratios and backgrounds that are not finite or not in [0, 1] -- inputs only a raw scene description holds, lights as stored records.
    The GPU tests (tests/test_raw_descriptor_gpu.py) take the oracle's word on them; here the reference renders them, two cameras."""
    s, twin, cams = _raw().named(name)
    ref = R.render(s, cams)
    for i, cam in enumerate(cams):
        bits_equal(s.render(cam=cam, nthreads=4), ref[i], f"{name} camera {i}")
    bits_equal(twin.render(cam=cams[0], nthreads=4), R.render(twin, cams[:1])[0], f"{name}, the twin")


@pytest.mark.parametrize("seed", _raw_seeds())
def test_raw_descriptor_generated_scenes(oracle, seed):
    """The seeded generator of the same module: the scene's own camera and the identity."""
    s, cam = _raw().scene(seed)
    cams = [cam, None]
    ref = R.render(s, cams)
    for i, c in enumerate(cams):
        bits_equal(s.render(cam=c, nthreads=4), ref[i], f"seed {seed} camera {i}")


def _own_edge_scenes(O):
    """Edges no builder above has: lights behind and on the surface, reflection_ratio at and around EPS, coincident objects,
    a scene with nothing in it, a hit exactly at EPS and at MAX_T."""
    def coefs(fn, *a):
        out = (C.c_double * 20)()
        getattr(O.lib(), fn)(*a, out)
        return list(out)

    def light(kind, intensity, v, color=(1.0, 1.0, 1.0)):
        l = O.OrcLight()
        getattr(O.lib(), "orc_light_" + kind)(float(intensity), O._d3(v), O._f3(color), C.byref(l))
        return l

    def base(w=48, h=36, depth=3):
        return O.Scene(w, h, 55.0, depth, (0.2, 0.3, 0.4))

    out = {}
    s = base()   # nothing at all
    out["no_objects_no_lights"] = s
    s = base()   # every light behind the lit side of the sphere, or pointing away from the plane
    s.add_object(coefs("orc_surface_sphere", O._d3((0, 0, 8)), 2.0), (0.9, 0.8, 0.7))
    s.add_object(coefs("orc_surface_plane", O._d3((0, -3, 0)), O._d3((0, 1, 0))), (0.5, 0.5, 0.5))
    s.lights += [light("directional", 1.0, (0, 0, -1)), light("directional", 1.0, (0, 1, 0)), light("spherical", 300.0, (0, -9, 8))]
    out["lights_behind_the_surface"] = s
    s = base()   # point lights on the sphere's surface, at its centre, and on the plane
    s.add_object(coefs("orc_surface_sphere", O._d3((0, 0, 8)), 2.0), (0.9, 0.8, 0.7))
    s.add_object(coefs("orc_surface_plane", O._d3((0, -3, 0)), O._d3((0, 1, 0))), (0.5, 0.5, 0.5))
    s.lights += [light("spherical", 50.0, (0, 0, 6)), light("spherical", 50.0, (0, 2, 8)), light("spherical", 50.0, (0, 0, 8)),
                 light("spherical", 50.0, (1, -3, 6))]
    out["point_lights_on_the_surface"] = s
    eps32 = np.float32(EPS)   # 1.00000001e-07: as a float it is ABOVE the double 1e-7 the reflection loop compares with
    for tag, ratio in (("below_eps", np.nextafter(eps32, np.float32(0))), ("at_eps", eps32), ("above_eps", np.nextafter(eps32, np.float32(1))),
                       ("one", 1.0), ("above_one", 1.5)):
        s = base()
        s.add_object(coefs("orc_surface_sphere", O._d3((-1.5, 0, 7)), 1.5), (0.9, 0.2, 0.2), ratio)
        s.add_object(coefs("orc_surface_sphere", O._d3((1.5, 0, 7)), 1.5), (0.2, 0.9, 0.2), ratio)
        s.add_object(coefs("orc_surface_plane", O._d3((0, -2, 0)), O._d3((0, 1, 0))), (0.5, 0.5, 0.5), ratio)
        s.lights += [light("directional", 1.0, (0.3, -1, 0.4)), light("spherical", 400.0, (0, 6, 2))]
        out["reflection_ratio_" + tag] = s
    s = base()   # coincident objects: the first of equal hits wins (t < best_t); each shadows the other
    for col in ((0.9, 0.1, 0.1), (0.1, 0.9, 0.1)):
        s.add_object(coefs("orc_surface_sphere", O._d3((0, 0, 8)), 2.0), col, 0.3)
    for col in ((0.1, 0.1, 0.9), (0.9, 0.9, 0.1)):
        s.add_object(coefs("orc_surface_plane", O._d3((0, -2.5, 0)), O._d3((0, 1, 0))), col)
    s.lights += [light("directional", 1.2, (0.3, -1, 0.4)), light("spherical", 400.0, (2, 6, 2))]
    out["coincident_objects"] = s
    # one pixel looks down +z: planes at exactly EPS and MAX_T and one double below / above (t >= EPS, t < MAX_T)
    for k, z in enumerate((EPS, np.nextafter(EPS, 0), MAX_T, np.nextafter(MAX_T, 0), np.nextafter(MAX_T, 2 * MAX_T))):
        s1 = base(1, 1)
        s1.add_object(coefs("orc_surface_plane", O._d3((0, 0, z)), O._d3((0, 0, 1))), (0.9, 0.8, 0.7))
        s1.lights.append(light("directional", 1.0, (0, 0, 1)))
        out[f"hit_at_bound_{k}"] = s1
    s = base()   # a wall that contains the light's direction in double (n . p == 0: no root) but not after the direction's round trip
    s.vertical_fov = O.lib().orc_radians(55.0)   # through float (|n . p| ~ 1e3 * 3e-8 > EPS: a root at distance / 3e-8), so that the
    lp = light("directional", 1.0, (0.3, -1.0, 0.4))   # floor within 0.03 of the wall, on one side of it, lies in its shadow
    s.add_object(coefs("orc_surface_plane", O._d3((0, -0.05, 0)), O._d3((0, 1, 0))), (1.0, 1.0, 1.0))
    s.add_object(coefs("orc_surface_plane", O._d3((0.02, 0, 0)), O._d3((1e3 * lp.p[1], -1e3 * lp.p[0], 0.0))), (0.9, 0.2, 0.2))
    s.lights.append(lp)
    out["shadow_direction_in_a_wall_but_for_float"] = s
    s = base()   # colours that sum past 1: the clamp comes once, after the sum over the lights
    s.add_object(coefs("orc_surface_sphere", O._d3((0, 0, 8)), 2.5), (1.0, 0.9, 0.8), 0.5)
    s.add_object(coefs("orc_surface_plane", O._d3((0, -2.5, 0)), O._d3((0, 1, 0))), (1.0, 1.0, 1.0))
    s.lights += [light("directional", 2.5, (0.3, -1, 0.4)), light("directional", 2.0, (-0.3, -1, 0.2)), light("spherical", 900.0, (0, 4, 5))]
    out["bright_lights"] = s
    return out


OWN_EDGES = ["no_objects_no_lights", "lights_behind_the_surface", "point_lights_on_the_surface", "reflection_ratio_below_eps",
             "reflection_ratio_at_eps", "reflection_ratio_above_eps", "reflection_ratio_one", "reflection_ratio_above_one", "coincident_objects",
             "hit_at_bound_0", "hit_at_bound_1", "hit_at_bound_2", "hit_at_bound_3", "hit_at_bound_4", "shadow_direction_in_a_wall_but_for_float",
             "bright_lights"]


@pytest.mark.parametrize("name", OWN_EDGES)
def test_constructed_edge_scenes(oracle, name):
    sc = _own_edge_scenes(oracle)[name]
    cams = [None, oracle.camera_matrix((0.4, 0.5, -1.0), 86.0, 3.0)] if sc.width > 1 else [None]
    ref = R.render(sc, cams)
    frames = [sc.render(cam=cam) for cam in cams]
    for want, got in zip(frames, ref):
        bits_equal(want, got, name)
    bg = np.asarray(sc.bg_color, dtype=np.float32)
    hit = bool((frames[0] != bg).any())
    if name.startswith("hit_at_bound_"):      # EPS: hit; below EPS: miss; MAX_T: miss; below MAX_T: hit; above MAX_T: miss
        assert hit == (name[-1] in "03"), name
    if name == "bright_lights":
        assert (frames[0] == 1.0).any(), "no channel reaches the clamp"
    if name == "shadow_direction_in_a_wall_but_for_float":   # white floor: lit, or black in the strip the float direction shadows
        floor = frames[0][:12]
        lit, dark = int((floor[..., 1] > 0.25).sum()), int((floor == 0).all(-1).sum())
        assert lit > 100 and 10 <= dark < lit, (lit, dark)
    if name.startswith("reflection_ratio_"):  # a float ratio of 1e-7 already mirrors; one float below it does not
        plain = _own_edge_scenes(oracle)[name]
        for o in plain.objects:
            o.reflection_ratio = 0.0
        assert np.array_equal(plain.render(), frames[0]) == name.endswith("below_eps"), name


# ---- 3. the functions, one call per row --------------------------------------------------------------------------------------
DP, FP = C.POINTER(C.c_double), C.POINTER(C.c_float)


def _dp(a):
    return a.ctypes.data_as(DP)


def oracle_intersect(O, rows):
    L, t, br = O.lib(), np.empty(len(rows)), np.empty(len(rows), dtype=np.int64)
    b = C.c_int(0)
    for i, r in enumerate(rows):
        t[i] = L.orc_intersect_ray_ex(_dp(r[:20]), _dp(r[20:23]), _dp(r[23:26]), None, C.byref(b))
        br[i] = b.value
    return t.reshape(-1, 1), br


def unit_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def shipped_coefs(O, name, index=0):
    return np.array(list(O.load_scene(scene_path(name)).objects[index].c))


def intersect_classes(O):
    """name -> rows [n, 26] (coef, origin, dir).  Random classes that reach every solver branch, then constructed edges."""
    rng = np.random.default_rng(20240)
    out = {}

    def rows(coef, o, d):
        n = max(np.atleast_2d(a).shape[0] for a in (coef, o, d))
        return np.ascontiguousarray(np.hstack([np.broadcast_to(np.atleast_2d(a), (n, np.atleast_2d(a).shape[1])) for a in (coef, o, d)]), dtype=np.float64)

    def sphere(c, r):
        k = np.zeros(20)
        k[10:13], k[16:19], k[19] = 1.0, -2.0 * np.asarray(c), np.dot(c, c) - r * r
        return k

    # random classes
    k = np.zeros((N, 20))
    k[:, 10:13] = 1.0
    c = rng.uniform([-6, -4, 4], [6, 4, 25], (N, 3))
    k[:, 16:19], k[:, 19] = -2.0 * c, (c * c).sum(1) - rng.uniform(0.3, 3.0, N) ** 2
    aim = c + rng.normal(size=(N, 3)) * rng.uniform(0.2, 3.0, (N, 1))
    o = rng.uniform(-2, 2, (N, 3))
    d = aim - o
    out["spheres"] = rows(k, o, d / np.linalg.norm(d, axis=1, keepdims=True))
    k = np.zeros((N, 20))   # general quadrics: both signs of t2, cross terms
    k[:, 10:13], k[:, 13:16] = rng.uniform(-2, 2, (N, 3)), rng.uniform(-1, 1, (N, 3)) * (rng.random((N, 1)) < 0.5)
    k[:, 16:19], k[:, 19] = rng.uniform(-20, 20, (N, 3)), rng.uniform(-60, 60, N)
    out["quadrics"] = rows(k, rng.uniform(-3, 3, (N, 3)), unit_dirs(rng, N))
    k = np.zeros((N, 20))   # planes; a tenth of the rays run inside a parallel plane (fabs(t1) <= EPS: no branch)
    nv = unit_dirs(rng, N)
    k[:, 16:19], k[:, 19] = nv, rng.uniform(-10, 10, N)
    d = unit_dirs(rng, N)
    par = np.cross(nv, d)
    par /= np.linalg.norm(par, axis=1, keepdims=True)
    d[::10] = par[::10]
    out["planes"] = rows(k, rng.uniform(-3, 3, (N, 3)), d)
    k = np.zeros((N, 20))   # random cubics, dense and sparse (tests/tools/fuzz_cubic.py's ranges)
    k[:, :10] = rng.uniform(-1, 1, (N, 10)) * (rng.random((N, 10)) < rng.uniform(0.2, 1.0, (N, 1)))
    k[:, 10:16], k[:, 16:19], k[:, 19] = rng.uniform(-1, 1, (N, 6)), rng.uniform(-2, 2, (N, 3)), rng.uniform(-4, 4, N)
    out["random_cubics"] = rows(k, rng.uniform(-8, 8, (N, 3)), unit_dirs(rng, N))
    for name in ("clebsch", "cayley", "dingdong", "monkey_saddle", "cubic"):
        out["shipped_" + name] = rows(shipped_coefs(O, name), rng.uniform(-3, 3, (N // 3, 3)), unit_dirs(rng, N // 3))
    d = unit_dirs(rng, N // 3).astype(np.float32).astype(np.float64)   # shadow rays: float directions, not normalised
    out["float_directions"] = rows(shipped_coefs(O, "clebsch"), rng.uniform(-2, 2, (N // 3, 3)), d * rng.uniform(0.1, 30, (N // 3, 1)))

    # constructed edges
    x3 = np.zeros(20)
    x3[0], x3[10:13], x3[18], x3[19] = 1.0, (1.0, 2.0, 1.0), -3.0, -4.0
    lead = []   # the leading coefficient: exactly 0, denormal, at EPS and one double either side, both signs
    for dx in (0.0, -0.0, 1e-110, 5e-108, -1e-105, EPS ** (1 / 3), np.cbrt(np.nextafter(EPS, 1)), np.cbrt(np.nextafter(EPS, 0)), -np.cbrt(EPS), 4.7e-3, 1e-2):
        for dz in (1.0, -1.0, 0.5):
            lead.append(np.concatenate([x3, (0.3, -0.2, -1.0), (dx, 0.1, dz)]))
    for s in (EPS, np.nextafter(EPS, 1), np.nextafter(EPS, 0), -EPS, -np.nextafter(EPS, 1), 5e-324, 1e-310):
        k = x3.copy()
        k[0] = s     # t3 = s exactly for dir = (1, 0, 0)
        lead.append(np.concatenate([k, (-3.0, 0.2, 0.1), (1.0, 0.0, 0.0)]))
        k = np.zeros(20)
        k[10], k[16], k[19] = s, 1.0, -2.0   # t2 = s: the quadratic / linear boundary
        lead.append(np.concatenate([k, (-3.0, 0.2, 0.1), (1.0, 0.0, 0.0)]))
        k = np.zeros(20)
        k[16], k[19] = s, -2.0 * s           # t1 = s: the linear / none boundary
        lead.append(np.concatenate([k, (-3.0, 0.2, 0.1), (1.0, 0.0, 0.0)]))
    out["leading_coefficient_edges"] = np.array(lead)
    tang = []   # discriminant exactly 0 and one float either side: rays tangent to spheres; triple and double roots of cubics
    for r in (1.0, 2.0, 0.5, 3.0):
        for z in (5.0, 8.0, 64.0):
            for off in (r, np.nextafter(r, 0), np.nextafter(r, 9), -r):
                tang.append(np.concatenate([sphere((0, 0, z), r), (off, 0, 0), (0, 0, 1.0)]))
                tang.append(np.concatenate([sphere((0, 0, z), r), (0, off, -3.0), (0, 0, 2.0)]))
    for root in (1.0, 2.0, 0.5, 3.0, -2.0):
        k = np.zeros(20)   # (x - root)^3 = 0 along x: q = r = delta = 0
        k[0], k[10], k[16], k[19] = 1.0, -3.0 * root, 3.0 * root * root, -root ** 3
        tang.append(np.concatenate([k, (0, 0, 0), (1.0, 0, 0)]))
        k = np.zeros(20)   # (x - root)^2 (x + 1): a double root, delta = 0 up to rounding
        k[0], k[10], k[16], k[19] = 1.0, 1.0 - 2.0 * root, root * root - 2.0 * root, root * root
        tang.append(np.concatenate([k, (0, 0, 0), (1.0, 0, 0)]))
        tang.append(np.concatenate([k, (-0.5, 0, 0), (2.0, 0, 0)]))
    out["tangents_and_multiple_roots"] = np.array(tang)
    k = -np.tile(sphere((0, 0, 6), 2.0), (N // 3, 1))   # negated spheres: t2 < 0, (-t1 - sqrt) / (2 t2) is the FAR root and comes first
    o = rng.uniform(-1, 1, (N // 3, 3))
    o[::3] = (0, 0, 6) + rng.normal(size=(len(o[::3]), 3)) * 0.5   # origin inside: the first candidate is negative, the second is taken whatever its sign
    out["negative_t2"] = rows(k, o, unit_dirs(rng, N // 3))
    out["behind_the_origin"] = rows(sphere((0, 0, -6), 2.0), rng.uniform(-1, 1, (N // 3, 3)), np.abs(unit_dirs(rng, N // 3)))   # both roots negative
    bound = []   # roots at EPS and MAX_T and next to them: planes, spheres through the origin region
    for z in (EPS, np.nextafter(EPS, 0), np.nextafter(EPS, 1), MAX_T, np.nextafter(MAX_T, 0), np.nextafter(MAX_T, 2e6), 0.0, -EPS):
        k = np.zeros(20)
        k[18], k[19] = 1.0, -z
        bound.append(np.concatenate([k, (0, 0, 0), (0, 0, 1.0)]))
        bound.append(np.concatenate([sphere((0, 0, z + 1.0), 1.0), (0, 0, 0), (0, 0, 1.0)]))    # near root at z
        bound.append(np.concatenate([sphere((0, 0, z - 1.0), 1.0), (0, 0, 0), (0, 0, 1.0)]))    # far root at z
    out["roots_at_the_bounds"] = np.array(bound)
    base = np.vstack([out["spheres"][:150], out["quadrics"][:150], out["planes"][:100], out["random_cubics"][:300]])
    for tag, s in (("1e150", 1e150), ("1e-150", 1e-150), ("1e300", 1e300), ("1e-300", 1e-300), ("5e-324", 5e-324)):
        r = base.copy()
        r[:, :20] *= s
        out["coefficients_times_" + tag] = r
    r = base.copy()
    r[:, 20:23] *= 1e90      # origins far out: t0 overflows, inf - inf
    out["origins_times_1e90"] = r
    r = base.copy()
    r[:, 23:26] *= 1e-60     # directions near zero
    out["directions_times_1e-60"] = r
    r = np.repeat(base[::7], 3, axis=0)   # an inf, a -inf or a NaN in one place of the row
    col = rng.integers(0, 26, len(r))
    r[np.arange(len(r)), col] = np.tile([np.inf, -np.inf, np.nan], len(r) // 3)
    out["inf_and_nan_inputs"] = r
    return out


BRANCH = {0: "none", 1: "linear", 2: "quadratic miss", 3: "quadratic hit", 4: "Cardano", 5: "trigonometric"}   # orc_intersect_ray_ex


def test_intersect_ray(oracle):
    """intersect_ray of the reference against orc_intersect_ray: random spheres, quadrics, planes, cubics and the shipped cubic
    surfaces, then constructed edges.  Every solver branch must have been reached by the random classes, and the edge classes must
    reach what they were built for."""
    classes = intersect_classes(oracle)
    reached = {}
    for name, rows in classes.items():
        want, br = oracle_intersect(oracle, rows)
        bits_equal(want, R.units("intersect_ray", rows), f"intersect_ray, class {name} ({len(rows)} rays)")
        reached[name] = {BRANCH[b]: int((br == b).sum()) for b in BRANCH}
    rnd = {b: sum(reached[c][b] for c in ("spheres", "quadrics", "planes", "random_cubics", "shipped_clebsch", "shipped_monkey_saddle")) for b in BRANCH.values()}
    assert all(n >= 100 for n in rnd.values()), rnd
    e = reached["leading_coefficient_edges"]
    assert all(e[b] > 0 for b in ("none", "linear", "quadratic hit")) and e["Cardano"] + e["trigonometric"] > 0, e
    t = classes["negative_t2"]
    want, br = oracle_intersect(oracle, t)
    assert np.all(br[want[:, 0] > 0] == 3) and (want[br == 3] < 0).any(), "no negative second candidate among the negated spheres"
    assert (oracle_intersect(oracle, classes["behind_the_origin"])[0] < 0).sum() > 100
    want, _ = oracle_intersect(oracle, classes["inf_and_nan_inputs"])
    assert np.isnan(want).any() and np.isfinite(want).any()
    assert sum(len(r) for r in classes.values()) > 15000


def test_normal_vector(oracle):
    """normal_vector at random points, at points ON the surfaces (from intersect_ray's roots), where the gradient vanishes (the
    shipped monkey saddle without its linear term on the y axis, Cayley's cubic at the origin: 0 * inf, NaN on both sides), and with
    huge, inf and NaN coordinates."""
    L = oracle.lib()
    classes = intersect_classes(oracle)
    rng = np.random.default_rng(20241)
    parts = []
    for name in ("spheres", "quadrics", "planes", "random_cubics", "shipped_clebsch", "shipped_cayley", "shipped_dingdong", "shipped_monkey_saddle", "shipped_cubic"):
        r = classes[name]
        t, _ = oracle_intersect(oracle, r)
        on = r[:, 20:23] + t * r[:, 23:26]
        parts += [np.hstack([r[:, :20], on]), np.hstack([r[:, :20], rng.uniform(-5, 5, (len(r), 3))])]
    saddle = shipped_coefs(oracle, "monkey_saddle")
    assert saddle[0] == 1.0 and saddle[6] == -3.0   # x^3 - 3 x z^2 (+ 10 y + 5 in the file)
    saddle[16:19] = 0.0
    pts = np.array([(0, 0, 0), (0.0, -0.0, 0.0), (5e-324, 0, 0), (1e-200, 1e-200, 0), (1e200, 1, 1), (np.inf, 0, 0), (np.nan, 1, 1), (1e-160, 0, 0)])
    edge = np.vstack([np.hstack([np.tile(k, (len(pts), 1)), pts]) for k in (saddle, shipped_coefs(oracle, "cayley"), shipped_coefs(oracle, "clebsch"), classes["spheres"][0, :20], np.zeros(20))])
    rows = np.ascontiguousarray(np.vstack(parts + [edge]))
    want = np.empty((len(rows), 3))
    for i, r in enumerate(rows):
        L.orc_normal_vector(_dp(r[:20]), _dp(r[20:23]), _dp(want[i]))
    bits_equal(want, R.units("normal_vector", rows), f"normal_vector ({len(rows)} points)")
    first = len(rows) - len(edge)
    assert np.isnan(want[first]).all() and np.isnan(want[first + len(pts)]).all(), "a zero gradient did not normalise to NaN"
    assert np.isfinite(want).all(axis=1).sum() > 10000


def _random_lights(rng, n):
    """[n, 7]: is_spherical, p (unit direction or a position), light_color (float values)."""
    sph = rng.random(n) < 0.5
    p = np.where(sph[:, None], rng.uniform(-20, 20, (n, 3)), unit_dirs(rng, n))
    col = (rng.uniform(0, 1, (n, 3)) * rng.uniform(0, 900, (n, 1))).astype(np.float32).astype(np.float64)
    return np.hstack([sph[:, None].astype(np.float64), p, col])


def _orc_light(O, row):
    l = O.OrcLight()
    l.is_spherical = int(row[0] != 0)
    for k in range(3):
        l.p[k], l.color[k] = row[1 + k], row[4 + k]
    return l


def test_shadow_ray(oracle):
    """shadow_ray returns a FLOAT vector: the direction light.p - surface_point makes one double -> float round trip, max_t is 1
    or 1e6.  Points near, far (a difference that overflows a float: inf) and with NaN."""
    L, rng = oracle.lib(), np.random.default_rng(20242)
    lights = _random_lights(rng, N)
    sp = rng.uniform(-30, 30, (N, 3))
    sp[::50] *= 1e38          # |p - sp| beyond FLT_MAX
    sp[1::50] = lights[1::50, 1:4] + rng.uniform(-1, 1, (N // 50, 3)) * 1e-42   # a difference that is a float denormal
    sp[2::50] = lights[2::50, 1:4]    # the point is the light
    sp[3::200, 0] = np.nan
    rows = np.ascontiguousarray(np.hstack([lights[:, :4], sp]))
    want = np.empty((N, 4))
    d, mt = (C.c_float * 3)(), C.c_double(0)
    for i, r in enumerate(rows):
        L.orc_shadow_ray(C.byref(_orc_light(oracle, lights[i])), _dp(sp[i]), d, C.byref(mt))
        want[i] = (d[0], d[1], d[2], mt.value)
    got = R.units("shadow_ray", rows)
    bits_equal(want, got, f"shadow_ray ({N} rays)")
    sph = rows[:, 0] != 0
    exact = rows[:, 1:4] - rows[:, 4:7]
    with np.errstate(over="ignore", invalid="ignore"):
        rounded = (got[sph, :3] != exact[sph]).any(axis=1).mean()
    assert rounded > 0.9, "the direction did not go through float"
    assert np.isinf(got[:, :3]).any() and set(np.unique(got[:, 3])) == {1.0, 1e6}


def test_surface_color(oracle):
    """surface_color: Lambert's max(0, n . l) clamp with back-facing normals (0), NaN normals (0, as (0 < NaN) is false), a point
    at the light (inf / NaN), inverse-square falloff in float."""
    L, rng = oracle.lib(), np.random.default_rng(20243)
    lights = _random_lights(rng, N)
    pt = rng.uniform(-15, 15, (N, 3))
    nrm = unit_dirs(rng, N)
    pt[::40] = lights[::40, 1:4]                       # the point is the light's position
    nrm[1::40] = np.nan
    nrm[2::40] *= 1e30
    col = rng.uniform(0, 1, (N, 3)).astype(np.float32).astype(np.float64)
    rows = np.ascontiguousarray(np.hstack([lights, pt, nrm, col]))
    want = np.empty((N, 3))
    o, c = (C.c_float * 3)(), (C.c_float * 3)()
    for i, r in enumerate(rows):
        c[0], c[1], c[2] = col[i]
        L.orc_surface_color(C.byref(_orc_light(oracle, lights[i])), _dp(pt[i]), _dp(nrm[i]), c, o)
        want[i] = (o[0], o[1], o[2])
    bits_equal(want, R.units("surface_color", rows), f"surface_color ({N} calls)")
    assert (want == 0).all(axis=1).sum() > N // 4 and (want > 1).any() and np.isnan(want).any()   # back-facing; beyond 1 (the clamp to 1 is the frame's)


def test_reflect_ray(oracle):
    L, rng = oracle.lib(), np.random.default_rng(20244)
    d, n = unit_dirs(rng, N), unit_dirs(rng, N)
    d[::30] *= 1e200
    n[1::30] = np.nan
    n[2::30] *= 1e-200
    rows = np.ascontiguousarray(np.hstack([d, n]))
    want = np.empty((N, 3))
    for i, r in enumerate(rows):
        L.orc_reflect_ray(_dp(r[:3]), _dp(r[3:6]), _dp(want[i]))
    bits_equal(want, R.units("reflect_ray", rows), f"reflect_ray ({N} rays)")


def test_surface_factories(oracle):
    """SurfaceCoefs::sphere / plane / dingDong / clebsch / cayley on random arguments (and large, tiny and zero ones); clebsch keeps
    the reference's z3 = 0 (surface.cpp assigns x3 twice)."""
    L, rng = oracle.lib(), np.random.default_rng(20245)
    scale = 10.0 ** rng.integers(-8, 9, (N, 1))

    def run(fn, rows, call):
        rows = np.ascontiguousarray(rows)
        want = np.empty((len(rows), 20))
        for i, r in enumerate(rows):
            call(r, _dp(want[i]))
        bits_equal(want, R.units(fn, rows), f"SurfaceCoefs::{fn} ({len(rows)} calls)")
        return want

    c = rng.uniform(-10, 10, (N, 3)) * scale
    c[::100] = 0.0
    run("sphere", np.hstack([c, np.abs(rng.uniform(0, 5, (N, 1)) * scale)]), lambda r, o: L.orc_surface_sphere(_dp(r[:3]), r[3], o))
    run("plane", np.hstack([c, rng.normal(size=(N, 3)) * scale[::-1]]), lambda r, o: L.orc_surface_plane(_dp(r[:3]), _dp(r[3:6]), o))
    run("dingDong", c, lambda r, o: L.orc_surface_dingdong(_dp(r[:3]), o))
    cl = run("clebsch", np.zeros((2, 1)), lambda r, o: L.orc_surface_clebsch(o))
    run("cayley", np.zeros((2, 1)), lambda r, o: L.orc_surface_cayley(o))
    assert cl[0, 2] == 0.0 and cl[0, 0] == cl[0, 1] == 81.0
    with pytest.raises(R.RefError, match="Negative value for sphere radius"):   # validate_positive: < 0 only
        R.units("sphere", [[0.0, 0.0, 0.0, -1.0]])
    assert R.units("sphere", [[0.0, 0.0, 0.0, 0.0]])[0, 19] == 0.0


def test_light_factories(oracle):
    """LightSource::directional (direction normalised in double and negated, colour times intensity in float) and spherical."""
    L, rng = oracle.lib(), np.random.default_rng(20246)
    inten = rng.uniform(0, 900, (N, 1)).astype(np.float32).astype(np.float64)
    inten[::60] = 0.0
    v = rng.normal(size=(N, 3)) * 10.0 ** rng.integers(-6, 7, (N, 1))
    v[1::60, :2] = 0.0             # along an axis
    v[2::60] *= 1e-160             # dot(v, v) underflows: 1 / sqrt(0)
    col = rng.uniform(0, 1, (N, 3)).astype(np.float32).astype(np.float64)
    col[3::60] = (0.0, 1.0, 1.0)
    rows = np.ascontiguousarray(np.hstack([inten, v, col]))
    for kind in ("directional", "spherical"):
        want = np.empty((N, 7))
        fn = getattr(L, "orc_light_" + kind)
        for i, r in enumerate(rows):
            l = oracle.OrcLight()
            fn(float(r[0]), _dp(v[i]), oracle._f3(col[i]), C.byref(l))
            want[i] = (l.is_spherical, *l.p, *l.color)
        bits_equal(want, R.units(kind, rows), f"LightSource::{kind} ({N} calls)")
    with pytest.raises(R.RefError, match="Negative value for light intensity"):
        R.units("directional", [[-1.0, 0, -1, 0, 1, 1, 1]])
    with pytest.raises(R.RefError, match="Invalid color"):
        R.units("spherical", [[1.0, 0, 1, 0, 1, 1.5, 1]])
