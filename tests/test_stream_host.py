"""The streamed frame kernel (RT_FLAG_STREAM, csrc/rt_stream.hip), host side: the ABI constants and symbols, the
refusals rt_create makes before it looks for a device (so they hold with or without a GPU), the build report's lines for the new
kernel, and -- on the oracle alone -- the conditions that keep the GPU tests (tests/test_stream_gpu.py) from being vacuous."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import stream_scenes as S  # noqa: E402


@pytest.fixture(autouse=True)
def the_feature(pkg):
    """The tests of the flag, the symbols, the refusals and the build report fail without the feature for their own reason.  The oracle-side
    conditions below are conditions OF the feature's GPU tests and say nothing without it, so they ask for it as well."""
    assert pkg.RT_FLAG_STREAM == 8192


def test_flag_in_header_and_binding(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"#define RT_FLAG_STREAM 8192u\b", hdr) and "#define RT_ABI_VERSION 3" in hdr
    assert pkg.RT_FLAG_STREAM == 8192
    others = (pkg.RT_FLAG_FAST | pkg.RT_FLAG_COUNT | pkg.RT_FLAG_SIMPLE | pkg.RT_FLAG_NOCULL | pkg.RT_FLAG_STATIC_ORDER | pkg.RT_FLAG_NOSCAN
              | pkg.RT_FLAG_PLAIN_ORDER | pkg.RT_FLAG_NOSPLIT | pkg.RT_FLAG_NOLEAN | pkg.RT_FLAG_SSAA2 | pkg.RT_FLAG_SSAA4 | pkg.RT_FLAG_SSAA_ADAPTIVE
              | pkg.RT_FLAG_SSAA_GEOMETRY | pkg.RT_MULTI_SELF_EXCHANGE | pkg.RT_MULTI_BANDWISE | pkg.RT_MULTI_SPARSE)
    assert not (others & pkg.RT_FLAG_STREAM)


def test_symbols_and_prototypes(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"\bint rt_get_streamed\(const rt_ctx \*ctx, uint32_t \*streamed\);", hdr)
    assert "rt_get_streamed" in pkg.ABI_SYMBOLS
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_get_streamed", "rt_launch_stream_strict", "rt_launch_stream_fast"):
        assert re.search(rf"\bT {sym}\b", names), sym
    lib = pkg.lib()
    assert lib.rt_get_streamed.argtypes[1] == C.POINTER(C.c_uint32)
    assert isinstance(pkg.Renderer.streamed, property)
    # the launcher is declared once, for both variants, and has its slot in the table the contexts call through
    launch = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc", "rt_launch.h")).read()
    assert re.search(r"RT_PER_VARIANT\(hipError_t, rt_launch_stream,", launch) and re.search(r"decltype\(&rt_launch_stream_strict\) stream;", launch)
    # null arguments need no device
    n = C.c_uint32(7)
    assert lib.rt_get_streamed(None, C.byref(n)) == -1 and b"rt_get_streamed" in lib.rt_last_error() and n.value == 7
    # the update.h adapter reads MI355RT_STREAM
    assert b"MI355RT_STREAM" in open(pkg.UPDATE_LIB_PATH, "rb").read()


def _create_rc(pkg, flags, name="quadratic"):
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(64, 48)
    d = sc.desc()
    cfg = pkg.Config(-1, 0, 1, 8, int(flags), pkg.RT_FMT_RGBA32F)
    ctx = C.c_void_p()
    rc = pkg.lib().rt_create(C.byref(ctx), C.byref(d), C.byref(cfg))
    if rc == 0:
        pkg.lib().rt_destroy(ctx)
    return rc, pkg.lib().rt_last_error().decode()


@pytest.mark.parametrize("other,word", [("RT_FLAG_SIMPLE", "RT_FLAG_SIMPLE"), ("RT_FLAG_COUNT", "counters"),
                                        ("RT_FLAG_SSAA2|RT_FLAG_SSAA_ADAPTIVE", "RT_FLAG_SSAA_ADAPTIVE"),
                                        ("RT_FLAG_SSAA4|RT_FLAG_SSAA_ADAPTIVE|RT_FLAG_SSAA_GEOMETRY", "RT_FLAG_SSAA_ADAPTIVE")])
def test_flag_only_refusals_come_before_the_device_query(pkg, other, word):
    """RT_ERR_INVALID (-1), never RT_ERR_NO_DEVICE (-4): the same answer on a machine without a GPU."""
    extra = 0
    for name in other.split("|"):
        extra |= getattr(pkg, name)
    for more in (0, pkg.RT_FLAG_FAST, pkg.RT_FLAG_NOCULL):
        rc, msg = _create_rc(pkg, pkg.RT_FLAG_STREAM | extra | more)
        assert rc == -1 and "RT_FLAG_STREAM" in msg and word in msg, (rc, msg)


def test_the_flag_alone_gets_past_the_checks(pkg):
    """Without a GPU rt_create gets as far as the device query; with one it creates the context."""
    import torch
    for extra in (0, pkg.RT_FLAG_SSAA2, pkg.RT_FLAG_FAST | pkg.RT_FLAG_NOCULL):
        rc, msg = _create_rc(pkg, pkg.RT_FLAG_STREAM | extra)
        assert rc in (0, -4), (rc, msg)
        if not torch.cuda.is_available():
            assert rc == -4


def test_build_report_lists_the_new_kernel_without_spills():
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    assert os.path.exists(report), "the library was not built by this tree's Makefile"
    lines = [l for l in open(report).read().splitlines() if "stream_frame_kernel" in l]
    for variant in ("strict", "fast"):
        mine = [l for l in lines if l.startswith(f"rt_stream_{variant}.o")]
        assert len(mine) == 4, mine   # <HAS_GQ, HAS_CUBIC>
    for l in lines:
        assert re.search(r"VGPR spills\s+0\s+scratch 0\b", l), l


def test_the_kernel_file_has_no_workgroup_barrier():
    """The waves of a workgroup run different numbers of bounces and chunks: nothing in the streamed kernel or its loops may wait for
    the other waves."""
    for name in ("rt_stream.hip", "rt_stream.hpp", "rt_stream_shade.hpp", "rt_stream_shell.hpp"):   # ... the shared loop and shell included
        text = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc", name)).read()
        code = "\n".join(l.split("//")[0] for l in text.splitlines())
        assert "__syncthreads" not in code and "s_barrier" not in code and "rq_stage_tables" not in code, name
        assert '"workgroup"' not in code and "extern __shared__" not in code and "HIP_DYNAMIC_SHARED" not in code, name
    assert "__builtin_amdgcn_wave_barrier" in open(os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc", "rt_stream.hpp")).read()


# ---- the conditions of the GPU tests, on the oracle alone ---------------------------------------------------------------------
def test_first_count_beyond_the_lds_limit_comes_from_the_launchers_rule(pkg):
    n = S.first_count_beyond_lds(pkg)
    f = pkg.lib().rt_wavefront_lds_bytes_strict
    assert f(n * 80, 2, 0, n, 0, 0) > S.LDS_LIMIT >= f((n - 1) * 80, 2, 0, n - 1, 0, 0)
    assert 1000 < n < 2600   # (the simple kernel's own limit is 160 KiB / 224 B = 731 objects: such a field is beyond both)
    # ... and the words are the ones rt_create forms for the field: 64 + 16 bytes per sphere behind the object records
    a = S.field(pkg, 70, 1).arrays()
    assert len(a["reflection"]) == 70 and not (a["coefs"][:, :16] != np.array([0] * 10 + [1, 1, 1, 0, 0, 0])).any()


@pytest.mark.parametrize("n", S.COUNTS)
def test_sphere_fields_show_their_first_last_and_highest_object(pkg, n):
    """In every sphere case an object of the first chunk, an object of the last chunk and the highest-index object each own a pixel --
    in the 64 x 48 frame and in the 37 x 21 one (partial tiles and blocks)."""
    for w, h in ((64, 48), (37, 21)):
        ow = S.Owners(S.oracle_of(pkg, S.field(pkg, n, S.FIELD_SEED, w=w, h=h)))
        last = ((n - 1) // S.CHUNK) * S.CHUNK
        assert ow.some_owner_in(0, min(S.CHUNK, n)) is not None, (n, w, h)
        assert ow.some_owner_in(last, n) is not None, (n, w, h)
        assert ow.pixel_of(n - 1) is not None, (n, w, h)


def test_large_field_shows_every_chunk_and_the_last_spheres_shadow(pkg):
    n = S.first_count_beyond_lds(pkg)
    sc = S.field(pkg, n, S.LARGE_SEED, big_last=True)
    osc = S.oracle_of(pkg, sc)
    ow = S.Owners(osc)
    for lo in range(0, n + 1, S.CHUNK):
        assert ow.some_owner_in(lo, min(lo + S.CHUNK, n + 1)) is not None, lo
    with_it, without = osc.render(nthreads=8), S.oracle_of(pkg, S.field(pkg, n, S.LARGE_SEED)).render(nthreads=8)
    changed = np.argwhere((with_it != without).any(axis=-1))
    assert any(ow.owner(int(x), int(y)) != n for y, x in changed[::7]), "the last sphere's shadow changes no pixel it does not own"


def test_large_mixed_scene_shows_every_chunk_of_both_tables(pkg):
    sc = S.mixed_large(pkg, 2000, S.MIXED_SEED)
    a = sc.arrays()
    osc = S.oracle_of(pkg, sc)
    ow = S.Owners(osc)
    sphere = [k for k in range(len(a["coefs"])) if (a["coefs"][k, 10:13] == 1.0).all() and not a["coefs"][k, 13:16].any()]
    plane = [k for k in range(len(a["coefs"])) if not a["coefs"][k, :16].any()]
    quadric = [k for k in range(len(a["coefs"])) if k not in set(sphere) and k not in set(plane)]
    assert len(sphere) == 1000 and len(quadric) == 1000 and len(plane) == 2 and (a["reflection"] > 0).sum() > 300 and a["max_reflections"] == 2
    for table in (sphere, quadric):
        for lo in range(0, len(table), S.CHUNK):
            assert any(ow.pixel_of(k) is not None for k in table[lo:lo + S.CHUNK]), lo
