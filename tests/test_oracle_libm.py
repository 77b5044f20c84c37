"""The oracle's cubic solver under another libm (oracle/rt_oracle.c, orc_libm_*; oracle.libm_hook / under_libm) and the device lab's
build (tests/tools/cubic_device_lab.hip).  No GPU: the "other libm" here is glibc itself, reached through the table, so every frame must
come out bit for bit as without the hook; what the table lacks must be a miss, never glibc's value."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

CUBIC = ["clebsch", "cayley", "cubic", "dingdong", "monkey_saddle"]
_LIBM = C.CDLL("libm.so.6")
for _f in ("cbrt", "acos", "cos"):
    getattr(_LIBM, _f).restype = C.c_double
    getattr(_LIBM, _f).argtypes = [C.c_double]


def glibc(name, args):
    f = getattr(_LIBM, name)
    return np.array([f(x) for x in np.asarray(args, dtype=np.float64).tolist()], dtype=np.float64)


def test_device_lab_cross_compiles_for_gfx950():
    import cubic_device_lab as D
    so = D.build(force=True)
    blob = open(so, "rb").read()
    assert b"gfx950" in blob
    for sym in (b"lab_libm", b"lab_rays", b"lab_guard"):
        assert sym in blob
    flags = D.devflags()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags   # (the Makefile's DEVFLAGS, read from the Makefile)


@pytest.mark.parametrize("name", CUBIC)
def test_glibc_through_the_table_gives_the_golden_frames(oracle, name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "frames_96x72.npz"))
    s = oracle.load_scene(scene_path(name)).with_size(96, 72)
    for cam in ("identity", "moved"):
        img, libm, rounds = oracle.under_libm(lambda: s.render(cam=g["cam_" + cam], nthreads=4), glibc)
        assert rounds == 1 and len(libm) > 0
        assert np.array_equal(img, g[f"{name}__{cam}"]), (name, cam)
    assert np.array_equal(s.render(cam=g["cam_moved"], nthreads=4), g[f"{name}__moved"])   # (and the hook is off again)


@pytest.mark.parametrize("name", CUBIC)
def test_record_mode_collects_no_more_arguments_than_the_branch_counters_imply(oracle, name):
    s = oracle.load_scene(scene_path(name)).with_size(96, 72)
    plain, cnt = s.render(counters=True, nthreads=4)
    with oracle.libm_hook("record") as h:
        img, cnt2 = s.render(counters=True, nthreads=4)
    assert np.array_equal(img, plain) and cnt2 == cnt
    # Cardano: two cube roots; trigonometric: one acos, three cosines -- distinct arguments may be fewer (duplicates), never more
    assert len(h.seen["cbrt"]) <= 2 * cnt["br_cardano"]
    assert len(h.seen["acos"]) <= cnt["br_trig"]
    assert len(h.seen["cos"]) <= 3 * cnt["br_trig"]
    assert (len(h.seen["cbrt"]) > 0) == (cnt["br_cardano"] > 0) and (len(h.seen["acos"]) > 0) == (cnt["br_trig"] > 0)


def _primary_tests(oracle, name, w=96, h=72):
    """(coefs, origin, dirs [n, 3]) of the primary rays of a one-object degree-3 scene."""
    s = oracle.load_scene(scene_path(name)).with_size(w, h)
    sc, cam = s.c_scene(), np.ascontiguousarray(oracle.IDENTITY)
    d = np.empty(3)
    dirs = []
    for y in range(h):
        for x in range(w):
            oracle.lib().orc_primary_dir(C.byref(sc), cam.ctypes.data_as(C.POINTER(C.c_double)), x, y, d.ctypes.data_as(C.POINTER(C.c_double)))
            dirs.append(d.copy())
    return np.ascontiguousarray(s.coefs[0]), np.zeros(3), np.array(dirs)


def _intersect_all(oracle, coefs, o, dirs):
    L, dp = oracle.lib(), C.POINTER(C.c_double)
    t, br = np.empty(len(dirs)), np.empty(len(dirs), dtype=np.int32)
    b = C.c_int(0)
    for i, d in enumerate(dirs):
        d = np.ascontiguousarray(d)
        t[i] = L.orc_intersect_ray_ex(coefs.ctypes.data_as(dp), o.ctypes.data_as(dp), d.ctypes.data_as(dp), None, C.byref(b))
        br[i] = b.value
    return t, br


def test_every_argument_the_table_lacks_is_a_miss(oracle):
    """Replace mode with an empty table: every argument is a miss (the same set record mode sees: the cube roots' arguments do not depend
    on the library) and every root that needs one is NaN.  With half the table: exactly the other half is missing."""
    coefs, o, dirs = _primary_tests(oracle, "clebsch")
    with oracle.libm_hook("record") as rec:
        t_ref, br_ref = _intersect_all(oracle, coefs, o, dirs)
    assert len(rec.seen["cbrt"]) > 100 and len(rec.seen["acos"]) > 100
    with oracle.libm_hook("replace", oracle.Libm()) as h:
        t, br = _intersect_all(oracle, coefs, o, dirs)
    for f in ("cbrt", "acos"):
        assert np.array_equal(h.seen[f].view(np.uint64), rec.seen[f].view(np.uint64)), f
    assert np.array_equal(br, br_ref)                               # (the branch is decided before any special function)
    special = (br == 4) | (br == 5)
    assert special.any() and np.isnan(t[special]).all() and np.array_equal(t[~special], t_ref[~special])
    half = oracle.Libm()
    keep = rec.seen["cbrt"][::2]
    half.add("cbrt", keep, glibc("cbrt", keep))
    for f in ("acos", "cos"):
        half.add(f, rec.seen[f], glibc(f, rec.seen[f]))
    with oracle.libm_hook("replace", half) as h:
        t, _ = _intersect_all(oracle, coefs, o, dirs)
    assert np.array_equal(h.seen["cbrt"].view(np.uint64), rec.seen["cbrt"][1::2].view(np.uint64))
    assert len(h.seen["acos"]) == 0 and len(h.seen["cos"]) == 0
    assert np.isnan(t[br == 4]).any() and np.array_equal(t[br == 5], t_ref[br == 5])


def test_under_libm_converges_and_repeats_what_it_was_given(oracle):
    """Values other than glibc's are used as given (cos made 1e-3 wrong moves the trigonometric roots and the frame), and under_libm
    converges though every new root brings new arguments."""
    s = oracle.load_scene(scene_path("clebsch")).with_size(48, 36)
    plain = s.render(nthreads=4)
    off = lambda name, a: glibc(name, a) * (1.0 + 1e-3) if name == "cos" else glibc(name, a)  # noqa: E731
    img, libm, rounds = oracle.under_libm(lambda: s.render(nthreads=4), off)
    assert 1 <= rounds <= 8
    assert not np.array_equal(img, plain)
    keys, vals = libm.tables["cos"]
    assert np.array_equal(vals, glibc("cos", keys.view(np.float64)) * (1.0 + 1e-3), equal_nan=True)
