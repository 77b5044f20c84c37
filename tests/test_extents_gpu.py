"""rt_object_extents / rt_object_extents_host / mi355rt_update_extents on the GPU (csrc/rt_gbuffer.hip).  The
reference is the numpy reduction (tests/tools/extents_ref.py) of the planes rt_render_gbuffer writes on the same context -- in every
build, degree 3 included -- and, for strict contexts and surfaces of degree <= 2, of the composer's planes.  Every comparison is on all
bits of the 40-byte records (t_min / t_max as uint64)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import extents_ref  # noqa: E402
from test_gpu_parity import mixed_scene, oracle_from, random_cubic_scene, random_scene  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 96, 72
MOVED = ((0.4, 0.3, -1.5), 84.0, -3.0)
US_ENTRY_BYTES = 64   # class-table bytes of one sphere (rt_scene_dev.h: UsEntry, held by a static_assert there)


def n_objects(r):
    return r._desc.n_objects


def from_planes(r, cam=None, rect=None):
    """The reduction of the planes rt_render_gbuffer writes on this context."""
    o, t, _, _ = r.gbuffer(cam, normal=False)
    return extents_ref.reduce_planes(o.cpu().numpy(), t.cpu().numpy(), n_objects(r), np.arange(r.width), r.row_map(), rect)


def assert_same(got, want, what=""):
    assert got.dtype == extents_ref.DTYPE == want.dtype and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        bad = [k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes()]
        raise AssertionError((what, f"{len(bad)} of {len(got)} records differ", [(k, got[k], want[k]) for k in bad[:4]]))


def check(r, cam=None, rect=None, what=""):
    got = r.object_extents(cam, rect)
    assert_same(got, from_planes(r, cam, rect), what)
    return got


def scenes(pkg):
    out = [(name, pkg.Scene.load_from_file(scene_path(name)).set_size(W, H), True) for name in ("20spheres", "quadratic", "reflection_test")]
    out.append(("mixed", mixed_scene(pkg, 5, w=W, h=H), True))
    out.append(("clebsch", pkg.Scene.load_from_file(scene_path("clebsch")).set_size(W, H), False))
    return out


# ---- 1, 2. against the planes and against the composer ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True])
def test_records_are_the_reduction_of_the_planes(pkg, fast):
    for name, sc, _ in scenes(pkg):
        r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_FAST if fast else 0)
        seen = 0
        for cam in (None, pkg.camera_matrix(*MOVED)):
            got = check(r, cam, what=(name, fast))
            seen += int((got["pixels"] > 0).sum())
        r.cleanup_update()
        assert seen > 0, name


def test_records_equal_the_composer(pkg, oracle):
    for name, sc, degree_two in scenes(pkg):
        if not degree_two:
            continue
        osc = oracle_from(pkg, oracle, sc)
        r = pkg.Renderer(sc, device=0)
        for cam, rect in ((None, None), (pkg.camera_matrix(*MOVED), (11, 9, 70, 50))):
            assert_same(r.object_extents(cam, rect), extents_ref.compose(osc, cam, rect), (name, rect))
        r.cleanup_update()


# ---- 3. rectangles -----------------------------------------------------------------------------------------------------------------------
def test_rectangles(pkg):
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(W, H)
    r = pkg.Renderer(sc, device=0)
    o, t, _, _ = r.gbuffer(normal=False)
    o, t = o.cpu().numpy(), t.cpu().numpy()
    ident = extents_ref.identity(n_objects(r))
    # a single pixel with an object: the record of rt_pick
    ys, xs = np.nonzero(o >= 0)
    x, y = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])
    got = check(r, rect=(x, y, x, y), what="one pixel")
    hit = r.pick([(x, y)])[0]
    k = int(hit["object"])
    assert k == o[y, x] and tuple(got[k])[:5] == (1, x, y, x, y)
    assert got["t_min"][k].view(np.uint64) == got["t_max"][k].view(np.uint64) == hit["t"].view(np.uint64)
    assert_same(np.delete(got, k), np.delete(ident, k), "the other objects of a one-pixel rectangle")
    # one tile; four tiles straddled, no edge on a multiple of 8; a rectangle on background; the full frame given explicitly
    tile = check(r, rect=(48, 32, 63, 47), what="tile")
    four = check(r, rect=(43, 29, 69, 51), what="four tiles")
    assert tile["pixels"].sum() > 0 and four["pixels"].sum() > tile["pixels"].sum()
    by, bx = np.nonzero(o < 0)
    bg = None
    for y0, x0 in zip(by.tolist(), bx.tolist()):   # the first 9 x 5 window without an object
        if x0 + 9 <= W and y0 + 5 <= H and np.all(o[y0:y0 + 5, x0:x0 + 9] < 0):
            bg = (x0, y0, x0 + 8, y0 + 4)
            break
    assert bg is not None
    assert_same(check(r, rect=bg, what="background"), ident, "background")
    assert_same(r.object_extents(rect=(0, 0, W - 1, H - 1)), r.object_extents(), "explicit full frame")
    assert int(r.object_extents()["pixels"].sum()) == int((o >= 0).sum())
    # what a context refuses: a rectangle that leaves the image, and supersampling
    for bad in ((0, 0, W, 0), (0, 0, 0, H), (W, 0, W, 0), (0, 0, 0xFFFFFFFF, 0)):
        with pytest.raises(pkg.RtError) as e:
            r.object_extents(rect=bad)
        assert e.value.code == -1 and "rect" in str(e.value)
    r.cleanup_update()
    import torch
    buf = torch.zeros((n_objects(r) * 5,), dtype=torch.int64, device="cuda:0")
    for fl in (pkg.RT_FLAG_SSAA2, pkg.RT_FLAG_SSAA4, pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA_ADAPTIVE, pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE):
        s = pkg.Renderer(sc, device=0, flags=fl)
        with pytest.raises(pkg.RtError) as e:
            s.object_extents()
        assert e.value.code == -1 and "rt_object_extents_host: not available for contexts created with RT_FLAG_SSAA2" in str(e.value)
        with pytest.raises(pkg.RtError) as e:
            s.object_extents_into(None, None, buf.data_ptr())
        assert e.value.code == -1 and "SSAA" in str(e.value)
        s.cleanup_update()


# ---- 4. odd sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(97, 71), (17, 9), (1, 1)])
def test_odd_sizes(pkg, w, h):
    for sc in (pkg.Scene.load_from_file(scene_path("quadratic")).set_size(w, h), mixed_scene(pkg, 3, w=w, h=h)):
        r = pkg.Renderer(sc, device=0)
        got = check(r, what=(w, h))
        check(r, pkg.camera_matrix(*MOVED), (0, 0, w - 1, h // 2), what=(w, h, "lower half"))
        check(r, rect=(w - 1, h - 1, w - 1, h - 1), what=(w, h, "last pixel"))
        r.cleanup_update()
        assert got["pixels"].sum() > 0 or (w, h) == (1, 1)   # (the one pixel of the mixed scene shows background)


# ---- 5. contention and the two accumulator paths -----------------------------------------------------------------------------------------
def test_one_sphere_fills_the_frame(pkg):
    sc = pkg.Scene.new(W, H, 50.0, 0, (0.0, 0.0, 0.0))
    sc.add_object(pkg.surface_make("sphere", [0, 0, 1.2], [1.0]), (1, 1, 1))
    r = pkg.Renderer(sc, device=0)
    got = check(r, what="one sphere")
    r.cleanup_update()
    assert tuple(got[0])[:5] == (W * H, 0, 0, W - 1, H - 1) and 0.2 - 1e-12 <= got["t_min"][0] < got["t_max"][0]


def lds_limit(pkg):
    """The largest sphere count whose accumulators still fit in LDS, from the launcher's own rule."""
    fn = pkg.lib().rt_extents_lds_accumulators_strict
    fn.argtypes = [C.c_size_t, C.c_uint32]
    lo, hi = 1, 4096
    assert fn(US_ENTRY_BYTES * lo, lo) == 1 and fn(US_ENTRY_BYTES * hi, hi) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fn(US_ENTRY_BYTES * mid, mid) else (lo, mid)
    return lo


@pytest.mark.parametrize("beyond", [0, 1])
def test_sphere_fields_at_the_switch_between_the_accumulator_paths(pkg, beyond):
    """The last scene with LDS accumulators and the first without: 64 x 48 frames of small spheres (extents_ref.sphere_field).  With the
    composer on the CPU, 1192 of 1575 and 1193 of 1576 objects (75.7 %) own a pixel, four at the most -- three times the quarter asked for."""
    n = lds_limit(pkg) + beyond
    sc = extents_ref.sphere_field(pkg, n, 7)
    for fl in (0, pkg.RT_FLAG_FAST):
        r = pkg.Renderer(sc, device=0, flags=fl)
        got = check(r, what=(n, fl))
        check(r, rect=(5, 3, 50, 40), what=(n, fl, "rectangle"))
        r.cleanup_update()
        assert int((got["pixels"] > 0).sum()) * 4 >= n


# ---- 6. ranks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_merge_to_the_whole_frame(pkg, world):
    sc = random_scene(pkg, 99, 14, 3, w=W, h=H)
    cam = pkg.camera_matrix(*MOVED)
    one = pkg.Renderer(sc, device=0)
    rects = (None, (10, 5, 80, 60), (0, 8, W - 1, 15))   # the last: the rows of rank 1's first band alone
    want = [one.object_extents(cam, rect) for rect in rects]
    one.cleanup_update()
    merged = [extents_ref.identity(len(want[0])) for _ in rects]
    for rank in range(world):
        r = pkg.Renderer(sc, device=0, rank=rank, world=world, band_rows=8)
        for k, rect in enumerate(rects):
            got = check(r, cam, rect, what=(world, rank, rect))
            if k == 2 and rank != 1:
                assert_same(got, extents_ref.identity(len(got)), "a rank without a row of the rectangle")
            merged[k] = extents_ref.merge(merged[k], got)
        r.cleanup_update()
    for k in range(len(rects)):
        assert_same(merged[k], want[k], (world, rects[k]))
    assert want[0]["pixels"].sum() > 0 and want[2]["pixels"].sum() > 0


# ---- 7. no frame state -------------------------------------------------------------------------------------------------------------------
def booked(counters):
    """tests_executed is left out: it is not a function of the frame sequence (tests/test_shade_gpu.py, booked)."""
    return {k: v for k, v in counters.items() if k != "tests_executed"}


def test_the_pass_is_invisible_to_the_frames(pkg):
    import torch
    w, h = 160, 90
    sc = random_scene(pkg, 4242, 40, 4, w=w, h=h, with_plane=False, mirrors=True)
    views = [pkg.camera_matrix((0.0, 0.0, 0.0), 90.0, 0.0), pkg.camera_matrix((0.0, 0.0, 0.0), -90.0, 0.0), pkg.camera_matrix((14.0, 2.0, 20.0), 160.0, -5.0)]
    fl = pkg.RT_FLAG_STRICT | pkg.RT_FLAG_COUNT
    fresh = pkg.Renderer(sc, device=0, flags=fl)
    want, want_cnt = [], []
    for cam in views:
        fresh.update(cam)
        want.append(fresh.download().copy())
        want_cnt.append(fresh.counters())
    fresh.cleanup_update()
    r = pkg.Renderer(sc, device=0, flags=fl)
    s2 = torch.cuda.Stream()
    dev = torch.zeros((n_objects(r) * 5,), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    first = r.object_extents(views[0])
    assert_same(first, from_planes(r, views[0]), "before any frame")
    for k, cam in enumerate(views):
        r.object_extents_into(views[(k + 1) % 3], None, dev.data_ptr(), stream=s2.cuda_stream, timed=False)   # a second stream, beside the frame
        r.update(cam)
        assert_same(r.object_extents(views[0]), first, k)
        assert np.array_equal(r.download().view(np.uint32), want[k].view(np.uint32)), k
        assert booked(r.counters()) == booked(want_cnt[k]), k
        s2.synchronize()
        assert_same(dev.cpu().numpy().view(extents_ref.DTYPE), from_planes(r, views[(k + 1) % 3]), ("second stream", k))
    for _ in range(10):
        r.update(views[2])
    assert_same(r.object_extents(views[0]), first, "after ten frames")
    r.cleanup_update()
    assert first["pixels"].sum() > 0


# ---- 8. with rt_set_scene ----------------------------------------------------------------------------------------------------------------
def test_scene_updates_and_one_graph(pkg):
    import torch
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(W, H)
    base = sc.arrays()
    steps = []
    for k in range(6):
        c = base["coefs"].copy()
        shift = np.array([0.4 * (k + 1), -0.25 * (k + 1), 0.5 * k])   # sphere 0 .. 2 move: x, y, z and the constant term
        for i in range(3):
            centre = -0.5 * c[i, 16:19]
            r2 = centre @ centre - c[i, 19]
            centre = centre + shift * (1 + i)
            c[i, 16:19] = -2.0 * centre
            c[i, 19] = centre @ centre - r2
        steps.append(c)

    def fresh(coefs):
        d = pkg.desc_from_arrays(**dict(base, coefs=coefs))
        f = pkg.Renderer(d, device=0)
        try:
            return f.object_extents()
        finally:
            f.cleanup_update()

    want = [fresh(c) for c in steps]
    assert want[0].tobytes() != want[1].tobytes()
    r = pkg.Renderer(sc, device=0)
    s = torch.cuda.Stream()
    try:
        r.set_scene(coefs=steps[0])
        assert_same(r.object_extents(), want[0], "after a moved sphere")
        assert_same(r.object_extents(), from_planes(r), "after a moved sphere, the planes")
        n = n_objects(r)
        with torch.cuda.stream(s):
            arrays = [torch.from_numpy(steps[k].copy()).to("cuda:0") for k in range(3)]
            outs = [torch.zeros((n * 5,), dtype=torch.int64, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        plain = []
        for k in range(6):   # the uncaptured calls, on the same stream
            with torch.cuda.stream(s):
                arrays[0].copy_(torch.from_numpy(steps[k].copy()))
            r.set_scene_into(coefs=arrays[0].data_ptr(), stream=s.cuda_stream)
            r.object_extents_into(None, None, outs[0].data_ptr(), stream=s.cuda_stream, timed=False)
            s.synchronize()
            plain.append(outs[0].cpu().numpy().view(extents_ref.DTYPE).copy())
            assert_same(plain[k], want[k], ("uncaptured", k))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):   # a serial chain on one stream
            for a, o in zip(arrays, outs):
                r.set_scene_into(coefs=a.data_ptr(), stream=s.cuda_stream)
                r.object_extents_into(None, None, o.data_ptr(), stream=s.cuda_stream, timed=False)
            with pytest.raises(pkg.RtError) as e:   # the host form allocates and waits
                r.object_extents(stream=s.cuda_stream)
            assert e.value.code == -1 and "capturing" in e.value.message
        for launch in range(2):
            with torch.cuda.stream(s):
                for k, a in enumerate(arrays):
                    a.copy_(torch.from_numpy(steps[3 * launch + k].copy()))
                for o in outs:
                    o.fill_(-1)
                g.replay()
            s.synchronize()
            for k, o in enumerate(outs):
                assert_same(o.cpu().numpy().view(extents_ref.DTYPE), plain[3 * launch + k], f"launch {launch}, call {k}")
        del g
    finally:
        torch.cuda.synchronize()
        r.cleanup_update()


# ---- 9. entry points ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_agree(pkg):
    import torch
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(W, H)
    cam = pkg.camera_matrix(*MOVED)
    rect = (9, 7, 77, 66)
    r = pkg.Renderer(sc, device=0)
    n = n_objects(r)
    host = r.object_extents(cam, rect)
    assert host.dtype == pkg.EXTENT_DTYPE and len(host) == n
    guard = 16
    dev = torch.full((n * 40 + guard,), 0xAB, dtype=torch.uint8, device="cuda:0")
    ms = r.object_extents_into(cam, rect, dev.data_ptr())
    assert ms is not None and ms > 0.0
    raw = dev.cpu().numpy()
    assert np.all(raw[n * 40:] == 0xAB), "bytes behind the records were written"
    assert_same(raw[:n * 40].view(extents_ref.DTYPE), host, "device entry")
    assert_same(host, from_planes(r, cam, rect), "host entry")
    with pytest.raises(pkg.RtError) as e:
        r.object_extents_into(cam, rect, dev.data_ptr() + 4)
    assert e.value.code == -1 and "aligned" in str(e.value)
    # ... while a host array may lie anywhere: the records are copied into it
    packed = np.zeros(n * 40 + 16, dtype=np.uint8)
    camc, rc4 = np.ascontiguousarray(cam, dtype=np.float64), np.array(rect, dtype=np.uint32)
    assert packed.ctypes.data % 8 == 0
    assert pkg.lib().rt_object_extents_host(r._h, camc.ctypes.data_as(C.POINTER(C.c_double)), rc4.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            C.c_void_p(packed.ctypes.data + 4), None) == 0, pkg.lib().rt_last_error()
    assert packed[4:4 + n * 40].tobytes() == host.tobytes() and not packed[:4].any() and not packed[4 + n * 40:].any()
    r.cleanup_update()
    # a scene without objects: RT_OK, nothing enqueued, nothing written
    empty = pkg.Scene.new(40, 30, 50.0, 2, (0.3, 0.6, 0.9))
    empty.add_light("directional", [0, -1, 0])
    r = pkg.Renderer(empty, device=0)
    assert len(r.object_extents()) == 0
    assert r.object_extents_into(None, None, dev.data_ptr(), timed=False) is None
    torch.cuda.synchronize()
    assert np.all(dev.cpu().numpy() == raw)
    r.cleanup_update()


def test_update_adapter_reports_the_last_frames_extents(pkg):
    """mi355rt_update_extents of libmi355rt_update.so through ctypes (as tests/test_set_scene_gpu.py drives mi355rt_update_scene)."""
    sc = pkg.Scene.load_from_file(scene_path("quadratic")).set_size(W, H)
    cam = np.ascontiguousarray(pkg.camera_matrix(*MOVED), dtype=np.float64)
    rect = np.array((9, 7, 77, 66), dtype=np.uint32)
    r = pkg.Renderer(sc, device=0)
    n = n_objects(r)
    want_full, want_rect = r.object_extents(cam), r.object_extents(cam, rect)
    r.cleanup_update()
    upd = C.CDLL(pkg.UPDATE_LIB_PATH)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    init = getattr(upd, re.search(r"\b(_Z\d+init_updatejRK5Scene)\b", names).group(1))
    update = getattr(upd, re.search(r"\b(_Z\d+updateRKN3glm3matI\S*)\b", names).group(1))
    cleanup = getattr(upd, re.search(r"\b(_Z\d+cleanup_updatev)\b", names).group(1))
    init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None
    update.argtypes, update.restype = [C.c_void_p], C.c_float
    upd.mi355rt_update_extents.argtypes = [C.POINTER(C.c_uint32), C.c_void_p, C.c_uint]
    err = pkg.lib().rt_last_error
    out = np.zeros(n, dtype=extents_ref.DTYPE)
    outp = C.c_void_p(out.ctypes.data)
    assert upd.mi355rt_update_extents(None, outp, n) == -1 and b"no update() call yet" in err()
    init(7, sc._h)
    try:
        assert upd.mi355rt_update_extents(None, outp, n) == -1 and b"no update() call yet" in err()
        update(cam.ctypes.data)
        assert upd.mi355rt_update_extents(None, outp, n + 1) == -1 and b"number of objects" in err()
        assert upd.mi355rt_update_extents(None, None, n) == -1 and b"null" in err()
        assert upd.mi355rt_update_extents(None, outp, n) == 0, err()
        assert_same(out, want_full, "update.h hook, full frame")
        assert upd.mi355rt_update_extents(rect.ctypes.data_as(C.POINTER(C.c_uint32)), outp, n) == 0, err()
        assert_same(out, want_rect, "update.h hook, rectangle")
    finally:
        cleanup()
    assert upd.mi355rt_update_extents(None, outp, n) == -1


def test_several_devices_are_refused_by_the_update_adapter(pkg):
    """MI355RT_DEVICES naming several devices: the multi-GPU layer has no extents entry.  A fresh process, for the environment."""
    code = ("import ctypes as C, re, subprocess, sys, numpy as np\n"
            "sys.path.insert(0, sys.argv[1])\nimport __graft_entry__ as g\npkg = g.load_package()\n"
            "sc = pkg.Scene.load_from_file(sys.argv[2]).set_size(96, 72)\nupd = C.CDLL(pkg.UPDATE_LIB_PATH)\n"
            "names = subprocess.run(['nm', '-D', '--defined-only', pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout\n"
            "init = getattr(upd, re.search(r'\\b(_Z\\d+init_updatejRK5Scene)\\b', names).group(1))\n"
            "update = getattr(upd, re.search(r'\\b(_Z\\d+updateRKN3glm3matI\\S*)\\b', names).group(1))\n"
            "cleanup = getattr(upd, re.search(r'\\b(_Z\\d+cleanup_updatev)\\b', names).group(1))\n"
            "init.argtypes, init.restype, cleanup.restype = [C.c_uint, C.c_void_p], None, None\nupdate.argtypes, update.restype = [C.c_void_p], C.c_float\n"
            "upd.mi355rt_update_extents.argtypes = [C.POINTER(C.c_uint32), C.c_void_p, C.c_uint]\n"
            "cam = np.ascontiguousarray(pkg.IDENTITY, dtype=np.float64)\nout = np.zeros(64, dtype=pkg.EXTENT_DTYPE)\n"
            "init(7, sc._h)\nupdate(cam.ctypes.data)\nrc = upd.mi355rt_update_extents(None, C.c_void_p(out.ctypes.data), sc.desc().n_objects)\n"
            "print(rc, pkg.lib().rt_last_error().decode())\ncleanup()\n")
    env = dict(os.environ, MI355RT_DEVICES="0,0")
    out = subprocess.run([sys.executable, "-c", code, ROOT, scene_path("quadratic")], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "-1 mi355rt_update_extents: not available with several devices (MI355RT_DEVICES)", out.stdout


def test_lds_refusal_names_the_entry_point(pkg):
    """Class tables beyond 160 KiB: 2561 spheres.  rt_create refuses such a scene for the product kernel, whose staging is larger, so the
    context is one of the simple kernel (RT_FLAG_SIMPLE), which stages nothing -- the one kind in which this refusal can be reached."""
    n = 160 * 1024 // US_ENTRY_BYTES + 1
    sc = extents_ref.sphere_field(pkg, n, 3, w=32, h=24)
    r = pkg.Renderer(sc, device=0, flags=pkg.RT_FLAG_SIMPLE)
    with pytest.raises(pkg.RtError) as e:
        r.object_extents()
    assert e.value.code == -2 and f"rt_object_extents_host: scene needs {n * US_ENTRY_BYTES} bytes of LDS per workgroup (limit 160 KiB)" in str(e.value)
    with pytest.raises(pkg.RtError) as e:
        r.gbuffer()
    assert e.value.code == -2 and "rt_render_gbuffer: scene needs" in str(e.value)
    r.cleanup_update()


# ---- 10. full size, once -----------------------------------------------------------------------------------------------------------------
def test_full_size(pkg):
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(1920, 1080)
    r = pkg.Renderer(sc, device=0)
    o, t, _, _ = r.gbuffer(normal=False)
    o, t = o.cpu().numpy(), t.cpu().numpy()
    got = r.object_extents()
    assert_same(got, extents_ref.reduce_planes(o, t, n_objects(r), np.arange(1920), np.arange(1080)), "1080p")
    assert int(got["pixels"].sum()) == int((o >= 0).sum()) > 10000
    r.cleanup_update()
