"""rt_debug_wave_box (the render kernel's box helper run alone, csrc/rt_wave_box.hpp / rt_wave_box.hip), host side: the prototype, the symbol,
the binding, and what the entry answers before it looks for a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")


def test_symbol_and_prototype(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"\bint rt_debug_wave_box\(rt_ctx \*ctx, const double \*pts, const uint64_t \*use_masks, uint32_t n_waves, float \*out\);", hdr)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_debug_wave_box", "rt_launch_wave_box"):
        assert re.search(rf"\bT {sym}\b", names), sym
    assert "rt_debug_wave_box" in pkg.ABI_SYMBOLS
    lib = pkg.lib()
    assert lib.rt_debug_wave_box.argtypes == [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_float)]
    assert callable(pkg.Renderer.wave_box)
    assert re.search(r'extern "C" hipError_t rt_launch_wave_box\(', open(os.path.join(CSRC, "rt_launch.h")).read())


def test_one_helper_for_both_schedules():
    """Both call sites of rt_wavefront.hip and the debug kernel call the one helper; the reductions it replaced are gone."""
    wf = open(os.path.join(CSRC, "rt_wavefront.hip")).read()
    assert len(re.findall(r"\bwave_box_f32\(", wf)) == 2
    assert not re.search(r"\bwave_(min|max)(_f)?\b|RT_WAVE_REDUCE|__double2float_r[du]", wf)
    assert len(re.findall(r"\bwave_box_f32\(", open(os.path.join(CSRC, "rt_wave_box.hip")).read())) == 1


def test_bad_arguments_are_refused_before_a_device_is_looked_for(pkg):
    lib = pkg.lib()
    pts = np.zeros((1, 64, 3))
    masks = np.zeros(1, dtype=np.uint64)
    out = np.full((1, 6), 9.0, dtype=np.float32)
    p, m, o = pts.ctypes.data_as(C.POINTER(C.c_double)), masks.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_float))
    # the checks below do not look into the context: any non-null handle does
    dummy = (C.c_uint64 * 4)()
    ctx = C.cast(dummy, C.c_void_p)
    for args in ((None, p, m, 1, o), (ctx, None, m, 1, o), (ctx, p, None, 1, o), (ctx, p, m, 1, None)):
        assert lib.rt_debug_wave_box(*args) == -1 and lib.rt_last_error() == b"rt_debug_wave_box: null argument"
    assert lib.rt_debug_wave_box(ctx, p, m, 0, o) == -1 and lib.rt_last_error() == b"rt_debug_wave_box: n_waves is 0"
    assert lib.rt_debug_wave_box(ctx, p, m, 65537, o) == -1 and b"exceeds 65536" in lib.rt_last_error()
    assert np.all(out == 9.0)
