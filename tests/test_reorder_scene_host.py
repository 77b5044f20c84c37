"""rt_reorder_scene (RT_FLAG_STREAM_CULL_REORDER, csrc/rt_reorder_scene.hip), host side: the ABI constant and symbols,
what the entry points answer before they look for a device, the launcher's declaration, the shared key function against its numpy
restatement (tests/tools/reorder_lab.py), and the conditions that keep the GPU tests from being vacuous: on each of their scenes the
order rt_set_scene leaves behind is not the fresh one, its bounds are wider and the frame's cones reach more of them."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import reorder_lab as RL  # noqa: E402

SC = RL.SC
CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(autouse=True)
def the_feature(pkg):
    """Everything here is about the feature."""
    assert pkg.RT_FLAG_STREAM_CULL_REORDER == 8388608


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_flag_in_header_and_binding(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"#define RT_FLAG_STREAM_CULL_REORDER 8388608u\b", hdr) and "#define RT_ABI_VERSION 3" in hdr
    assert pkg.RT_FLAG_STREAM_CULL_REORDER == 8388608 == 0x800000 == 2 * pkg.RT_FLAG_STREAM_CULL_PIXELS
    names = set(re.findall(r"#define (RT_FLAG_\w+|RT_MULTI_\w+) (?:0x[0-9a-fA-F]+|\d+)u\b", hdr))
    assert "RT_FLAG_STREAM_CULL_REORDER" in names
    for name in names - {"RT_FLAG_STREAM_CULL_REORDER"}:
        assert not (getattr(pkg, name) & pkg.RT_FLAG_STREAM_CULL_REORDER), name
    assert "reorder = RT_FLAG_STREAM_CULL_REORDER && rt_get_stream_cull" in hdr
    updates = hdr.split("Scene updates: move objects and lights of a live context")[1].split("typedef struct rt_scene_update")[0]
    for word in ("Re-sorting (RT_FLAG_STREAM_CULL_REORDER", "rt_set_scene never changes", "a chunk is finite or infinite after a reorder exactly as",
                 "`(rt_set_scene, rt_reorder_scene, rt_render) x K` can be captured once and replayed", "no allocation, no host read-back, no wait"):
        assert word in updates, word
    assert "which was chosen at rt_create and stays" not in hdr


def test_symbols_and_prototypes(pkg):
    hdr = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert re.search(r"\bint rt_reorder_scene\(rt_ctx \*ctx, void \*stream\);", hdr)
    assert re.search(r"\bint rt_get_stream_cull_reorder\(const rt_ctx \*ctx, uint32_t \*on\);", hdr)
    assert re.search(r"\bint rt_reorder_scene_multi\(rt_multi \*m\);", hdr)
    names = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("rt_reorder_scene", "rt_get_stream_cull_reorder", "rt_launch_reorder_scene", "rt_reorder_scene_work_size"):
        assert re.search(rf"\bT {sym}\b", names), sym
    assert "rt_reorder_scene" in pkg.ABI_SYMBOLS and "rt_get_stream_cull_reorder" in pkg.ABI_SYMBOLS
    multi = subprocess.run(["nm", "-D", "--defined-only", pkg.MULTI_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rt_reorder_scene_multi\b", multi) and "rt_reorder_scene_multi" in pkg.MULTI_ABI_SYMBOLS
    assert isinstance(pkg.Renderer.stream_cull_reorder, property) and callable(pkg.Renderer.reorder_scene) and callable(pkg.MultiRenderer.reorder_scene)
    import inspect
    for fn in (pkg.Renderer.set_scene, pkg.Renderer.set_scene_into):
        assert inspect.signature(fn).parameters["reorder"].default is False
    update = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "host", "src", "update-hip.cpp")).read()
    assert 'std::getenv("MI355RT_STREAM_CULL_REORDER")' in update and 'die_text("MI355RT_STREAM_CULL_REORDER", "expected 0 or 1")' in update


def test_null_arguments_are_refused_before_a_device_is_looked_for(pkg):
    lib = pkg.lib()
    n = C.c_uint32(7)
    assert lib.rt_reorder_scene(None, None) == -1 and b"rt_reorder_scene: null argument" in lib.rt_last_error()
    assert lib.rt_get_stream_cull_reorder(None, C.byref(n)) == -1 and b"rt_get_stream_cull_reorder: null argument" in lib.rt_last_error()
    assert n.value == 7
    assert pkg.multi_lib().rt_reorder_scene_multi(None) == -1 and b"rt_reorder_scene_multi: null argument" in lib.rt_last_error()
    # (a NULL `on` with a context: the check stands in front of everything else in the function)
    capi = open(os.path.join(CSRC, "rt_capi.cpp")).read()
    body = capi.split('extern "C" int rt_get_stream_cull_reorder(const rt_ctx *ctx, uint32_t *on)')[1].split("}")[0]
    assert body.lstrip("\n {").startswith('if (!ctx || !on) return fail(RT_ERR_INVALID, "rt_get_stream_cull_reorder: null argument");')
    body = capi.split('extern "C" int rt_reorder_scene(rt_ctx *ctx, void *stream_)')[1]
    assert body.index("if (!ctx) return fail(RT_ERR_INVALID") < body.index("if (!ctx->reorder) return RT_OK;") < body.index("use_device(ctx)")


def test_the_launcher_is_declared_once_beside_set_scene(pkg):
    launch = open(os.path.join(CSRC, "rt_launch.h")).read()
    decl = 'extern "C" hipError_t rt_launch_reorder_scene(void *t_us, uint32_t n_us, uint32_t n_obj, void *bounds, void *work, uint32_t max_grid, hipStream_t stream);'
    assert launch.count(decl) == 1 and launch.count("rt_launch_reorder_scene") == 1
    assert launch.index("rt_launch_set_scene(") < launch.index(decl) < launch.index("enum TablePath")
    assert not re.search(r"RT_PER_VARIANT\([^)]*reorder", launch)
    assert 'extern "C" size_t rt_reorder_scene_work_size(uint32_t n_us);' in launch
    src = open(os.path.join(CSRC, "rt_reorder_scene.hip")).read()
    assert '#include "rt_launch.h"' in src and "rtp::stream_cull_key(" in src and "rtp::pack_chunk_bound(" in src
    # one copy of the key rule: the host's packer calls the function the kernel calls
    image = open(os.path.join(CSRC, "rt_scene_image.hpp")).read()
    assert "stream_cull_key(old[j], lo, hi)" in image and "2097151" not in "\n".join(l.split("//")[0] for l in image.splitlines())
    mk = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "Makefile")).read()
    rule = next(l for l in mk.splitlines() if l.startswith("$(BUILD)/csrc/rt_resolve.o") and "%.hip" in l)
    assert "$(BUILD)/csrc/rt_reorder_scene.o" in rule and "$(BUILD)/csrc/rt_reorder_scene.o" in next(l for l in mk.splitlines() if l.startswith("OBJ "))


# ---- the key ----------------------------------------------------------------------------------------------------------------------------
def agree(e, lo, hi):
    got, want = RL.keys(e, lo, hi), RL.keys_numpy(e, lo, hi)
    assert np.array_equal(got, want), int((got != want).sum())
    return got


def test_key_function_on_random_inputs():
    rng = np.random.default_rng(11)
    for scale in (1e-3, 1.0, 1e6, 1e150):
        c = rng.normal(scale=scale, size=(4000, 3))
        r = np.where(rng.random(4000) < 0.1, np.inf, rng.uniform(0.1, 2.0, 4000))
        e = RL.entries(c, r)
        lo, hi = RL.box_of(e)
        k = agree(e, lo, hi)
        assert (k[r == np.inf] == ALL).all() and (k[r < np.inf] < (np.uint64(1) << np.uint64(63))).all()
        # a box that is not the entries' own: the clamps on both sides
        agree(e, lo * 0.5 + 0.1 * scale, hi * 0.5)


def test_key_function_on_the_edges():
    rng = np.random.default_rng(12)
    c = rng.uniform(-5, 5, (200, 3))
    r = np.ones(200)
    # hi == lo on one axis, and on all: the axis contributes no bit
    flat = c.copy()
    flat[:, 1] = 0.75
    e = RL.entries(flat, r)
    k = agree(e, *RL.box_of(e))
    y_bits = sum(np.uint64(1) << np.uint64(3 * b + 1) for b in range(21))
    assert not (k & y_bits).any() and k.any()
    e = RL.entries(np.tile([1.0, -2.0, 3.0], (200, 1)), r)
    assert not agree(e, *RL.box_of(e)).any()
    # zero spans of either sign, and zeros of either sign in lo: the same keys (what lets the device reduce the box in any order)
    e = RL.entries(np.array([[0.0, 1.0, -0.0], [-0.0, 2.0, 0.0], [0.0, 3.0, 0.0]]), np.ones(3))
    want = agree(e, [0.0, 1.0, 0.0], [0.0, 3.0, 0.0])
    for lo0 in (0.0, -0.0):
        for hi0 in (0.0, -0.0):
            assert np.array_equal(agree(e, [lo0, 1.0, -lo0], [hi0, 3.0, -hi0]), want)
    assert not (want & ~y_bits).any()
    # an infinite span: no bit; a NaN span likewise
    e = RL.entries(c, r)
    lo, hi = RL.box_of(e)
    big_lo, big_hi = lo.copy(), hi.copy()
    big_lo[0], big_hi[0] = -1.7e308, 1.7e308
    x_bits = y_bits << np.uint64(1)
    assert not (agree(e, big_lo, big_hi) & x_bits).any()
    big_hi[0] = np.nan
    assert not (agree(e, big_lo, big_hi) & x_bits).any()
    # the largest quantum: the entry at hi gets 2 097 151 on that axis, the one at lo 0
    k = agree(e, lo, hi)
    for axis in range(3):
        bits = sum(np.uint64(1) << np.uint64(3 * b + (2 - axis)) for b in range(21))
        assert (k[np.argmax(c[:, axis])] & bits) == bits and (k[np.argmin(c[:, axis])] & bits) == 0
    assert int(RL.QMAX) == (1 << 21) - 1
    # duplicate centres: equal keys (the order then goes by orig); an entry without a radius: ~0 whatever its centre
    dup = np.concatenate([c[:50], c[:50]])
    e = RL.entries(dup, np.ones(100))
    k = agree(e, *RL.box_of(e))
    assert np.array_equal(k[:50], k[50:])
    e["r"][7] = np.inf
    e["k"][7] = np.nan
    assert agree(e, lo, hi)[7] == ALL


def test_the_numpy_order_is_the_packers(pkg):
    """reorder_lab.order_numpy == the order stream_cull_image gives the table, on a scene with ties and unbounded spheres."""
    sc = RL.base_scene(pkg, 320, RL.UNBOUNDED_AT)
    a = sc.arrays()
    for coefs in (a["coefs"], RL.mix(a["coefs"], unbounded=RL.UNBOUNDED_AT), RL.ties(a["coefs"], "two")):
        plain, _, w = SC.image(dict(a, coefs=coefs), ordered=False)
        blob, _, _ = SC.image(dict(a, coefs=coefs))
        t0, t = SC.table_of(plain, w), SC.table_of(blob, w)
        assert np.array_equal(t0[RL.order_numpy(t0)].view(np.uint8), t.view(np.uint8))
        # ... and from any starting order, as the device meets it
        shuffled = t0[np.random.default_rng(3).permutation(len(t0))]
        assert np.array_equal(shuffled[RL.order_numpy(shuffled)].view(np.uint8), t.view(np.uint8))


# ---- the conditions of the GPU tests ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conditions_of(pkg, n, mirrors=False, depth=0):
    ub = RL.UNBOUNDED_AT if n == 320 else ()
    sc = RL.base_scene(pkg, n, ub, mirrors=mirrors, depth=depth)
    return RL.conditions(pkg, sc, RL.mix(sc.arrays()["coefs"], unbounded=ub))


@pytest.mark.parametrize("n", RL.SIZES + (RL.MANY,))
def test_the_mixed_scenes_lose_their_order(pkg, n):
    """Bytes, frames, work words, graph, consumers, multi: S0 = base_scene(n), S1 = mix.  A table of one chunk (64) has one bound whatever the
    order -- pack_chunk_bound is a function of the member set -- so there only the bytes can differ; from two chunks on the stale bounds
    are wider and the block cones reach strictly more of them."""
    c = conditions_of(pkg, n)
    print(n, c)
    assert c["differs"]
    if n > 64:
        assert c["stale_radii"] > c["fresh_radii"] and c["stale_reached"] > c["fresh_reached"], c


def test_the_consumer_scene_loses_its_order(pkg):
    c = conditions_of(pkg, 129, True, 2)
    assert c["differs"] and c["stale_radii"] > c["fresh_radii"] and c["stale_reached"] > c["fresh_reached"], c


@pytest.mark.parametrize("kind", ["two", "plane", "identical"])
def test_the_tie_scenes_differ_from_the_fresh_image(pkg, kind):
    """65 spheres on two centres / in one plane / on one centre: held to bytes only on the GPU, so the bytes must differ here.  (All centres
    identical: every chunk has the same bound under any order, so there is no wider bound to ask for.)"""
    sc = RL.base_scene(pkg, 65)
    a = sc.arrays()
    coefs = RL.ties(a["coefs"], kind)
    sb, sbounds, w = RL.stale(a, coefs)
    fb, fbounds, _ = RL.fresh(a, coefs)
    assert not np.array_equal(sb, fb)
    t = SC.table_of(fb, w)
    if kind == "identical":
        assert np.array_equal(t["orig"], np.arange(65))
    if kind == "two":
        lo, hi = RL.box_of(t)
        assert len(set(RL.keys(t, lo, hi).tolist())) == 2


def test_a_false_decision_scene_has_no_chunks_to_order(pkg):
    """Three cullable spheres: culling is off (fewer than four), so RT_FLAG_STREAM_CULL's decision and with it the reorder decision is false."""
    _, _, w = SC.image(RL.base_scene(pkg, 3).arrays())
    assert w["cull"] == 0
