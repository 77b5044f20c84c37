"""Raw-descriptor inputs on the GPU: scenes that rt_create accepts from a raw rt_scene_desc but no scene factory can produce
(tests/tools/raw_desc_scenes.py) -- directional lights of any length (short, zero, long, NaN, inf), light colours, albedos, reflection
ratios and backgrounds that are not finite or not in [0, 1].  rt_create clears backface_exact / the quadratic-branch bit / lights_plain
on them, and the kernels then run arms no other test reaches (the general light loop of the lean path and its four (bfe, quad_l)
combinations, the same pair in phase B of the general instantiation, the counting builds' bookkeeping under bfe = 0).

Every frame of degree <= 2 is compared on its bit pattern (np.array_equal calls -0.0 and 0.0 equal; both occur here): between the
kernels exactly, against the oracle with the one allowance that a NaN channel has to be a NaN on both sides (the device and glibc
spell NaN differently).  tests/test_oracle_vs_reference.py holds the oracle to the reference's CPU build on the same scenes.  The
degree-3 scenes keep the bars of test_random_cubic_scenes_within_tolerance, and their counters those of test_degree_three_counters.

RGBA8 is held exactly: the byte is the low byte of (int) ((v * 255.0f) + 0.5f), each operation rounded to float, v the RGBA32F channel
of the same kind of context; asserted wherever v is finite and |v * 255| < 2^31, alpha 255."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cubic_device_lab as D  # noqa: E402
import gbuffer_ref  # noqa: E402
import raw_desc_scenes as S  # noqa: E402
import ssaa_adaptive_ref as ada  # noqa: E402
import ssaa_geometry_ref as geo  # noqa: E402
import ssaa_ref  # noqa: E402
from raw_desc_scenes import n_diff, render_desc, same, same_as_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

F32, U8 = 0, 1
COUNTED = ("primary_rays", "shadow_rays", "reflect_rays", "tests", "hits")
CASES = [("named", n) for n in S.NAMED] + [("seed", s) for s in range(S.N_SEEDS)]


def case_id(key):
    return f"{key[0]}-{key[1]}"


def build(key):
    """(oracle scene, camera): a named scene under one of its two cameras (by its place in the list), or a generated one."""
    if key[0] == "named":
        s, _, cams = S.named(key[1])
        return s, cams[list(S.NAMED).index(key[1]) % 2]
    return S.scene(key[1])


def rgba8_of(v):
    """(expected RGBA8 [..., 4], mask of the channels that have an expectation) of an RGBA32F frame."""
    v = np.ascontiguousarray(v[..., :3], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        m = v * np.float32(255.0)
        t = m + np.float32(0.5)
        ok = np.isfinite(v) & (np.abs(m.astype(np.float64)) < 2.0 ** 31) & (np.abs(t.astype(np.float64)) < 2.0 ** 31)
        q = np.where(ok, t, np.float32(0.0)).astype(np.int32)     # (int): truncation towards zero
    out = np.empty(v.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = (q & 0xFF).astype(np.uint8)                    # (unsigned char): the low byte
    out[..., 3] = 255
    return out, ok


def check_rgba8(got8, v32, what):
    want, ok = rgba8_of(v32)
    assert got8.dtype == np.uint8 and np.all(got8[..., 3] == 255), what
    bad = (got8[..., :3] != want[..., :3]) & ok
    assert not bad.any(), f"{what}: {int(bad.sum())} RGBA8 channels differ from (int) (v * 255 + 0.5)"


def variants(pkg):
    return [("default", 0), ("nocull", pkg.RT_FLAG_NOCULL), ("simple", pkg.RT_FLAG_SIMPLE)]


# ---- 1. frames of every kernel variant ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_kernel_variants_and_oracle(pkg, oracle, key, monkeypatch):
    """Default, RT_FLAG_NOCULL and RT_FLAG_SIMPLE (three frames per context: launch-order feedback active), on sphere-only scenes also
    the lean instantiation forced (MI355RT_LEAN=always) against RT_FLAG_NOLEAN, in RGBA32F and RGBA8: the same bits from all of them,
    the oracle's in RGB, and RGBA8 exactly the stated rounding of the RGBA32F frame.  The FMA-contracted build: lean == general."""
    monkeypatch.delenv("MI355RT_LEAN", raising=False)
    osc, cam = build(key)
    cls = S.scene_class(osc)
    d = S.desc(pkg, osc)
    fr = {n: render_desc(pkg, d, cam, flags=f) for n, f in variants(pkg)}
    fr8 = {n: render_desc(pkg, d, cam, flags=f, fmt=pkg.RT_FMT_RGBA8) for n, f in variants(pkg)}
    if cls in S.SPHERE_ONLY:
        monkeypatch.setenv("MI355RT_LEAN", "always")
        fr["lean"] = render_desc(pkg, d, cam)
        fr8["lean"] = render_desc(pkg, d, cam, fmt=pkg.RT_FMT_RGBA8)
        fr["nolean"] = render_desc(pkg, d, cam, flags=pkg.RT_FLAG_NOLEAN)
        fr8["nolean"] = render_desc(pkg, d, cam, flags=pkg.RT_FLAG_NOLEAN, fmt=pkg.RT_FMT_RGBA8)
        fast = render_desc(pkg, d, cam, flags=pkg.RT_FLAG_FAST)
        assert same(fast, render_desc(pkg, d, cam, flags=pkg.RT_FLAG_FAST | pkg.RT_FLAG_NOLEAN)), "FMA-contracted build: lean and general instantiation disagree"
    a = fr["default"]
    want = osc.render(cam=cam, nthreads=8)
    print(f"{case_id(key)}: class {cls}, flags {S.flags(osc)[2:]}, pixels off the oracle " +
          ", ".join(f"{n} {n_diff(np.where(np.isnan(v[..., :3]), np.float32(0), v[..., :3]), np.where(np.isnan(want), np.float32(0), want))}" for n, v in fr.items()))
    for n, v in fr.items():
        assert same(a, v), f"default and {n} disagree on {n_diff(a, v)} pixels"
    assert np.array_equal(a[..., 3].view(np.uint32), np.full(a.shape[:2], 0x3F800000, dtype=np.uint32))
    if cls == "cubic":   # the bars of test_random_cubic_scenes_within_tolerance
        c = compare(a[..., :3], want)
        assert c["n_bad_pixels"] <= max(3, int(0.002 * osc.width * osc.height)), c
        c = D.compare_device_libm(pkg, a[..., :3], osc, cam=cam)
        assert c["n_bad_pixels"] == 0, c
    else:
        assert same_as_oracle(a[..., :3], want), f"{n_diff(a[..., :3], want)} pixels differ from the oracle"
    for n, v in fr8.items():
        assert np.array_equal(fr8["default"], v), f"RGBA8: default and {n} disagree"
        check_rgba8(v, fr[n], n)


# ---- 2. the counting builds ----------------------------------------------------------------------------------------------------
def counting_frames(pkg, d, cam, flags, n=2):
    """[(counters, frame)] of n frames of one counting context."""
    r = pkg.Renderer(d, device=0, flags=flags | pkg.RT_FLAG_COUNT)
    try:
        out = []
        for _ in range(n):
            r.update(cam)
            out.append((r.counters(), r.download().copy()))
        return out
    finally:
        r.cleanup_update()


@pytest.mark.parametrize("key", [k for k in CASES if k[0] == "seed" or S.NAMED[k[1]][0] != "cubic"], ids=case_id)
def test_counters(pkg, oracle, key, monkeypatch):
    """RT_FLAG_COUNT, on sphere-only scenes lean forced and RT_FLAG_NOLEAN (elsewhere the two are the same instantiation: one context):
    the counters test_counters_fuzz_gpu holds to the oracle (hits: its `normals`), and the counting build's frame is the product
    frame.  With bfe = 0 every lane with a hit is `wanted`: the bookkeeping of the counting light loops runs with lanes it never saw."""
    monkeypatch.setenv("MI355RT_LEAN", "always")
    osc, cam = build(key)
    d = S.desc(pkg, osc)
    _, want = osc.render(cam=cam, counters=True, nthreads=8)
    want = dict(want, hits=want["normals"])
    product = render_desc(pkg, d, cam, flags=pkg.RT_FLAG_NOLEAN)
    for fl in ((0, pkg.RT_FLAG_NOLEAN) if S.scene_class(osc) in S.SPHERE_ONLY else (0,)):
        for frame, (got, img) in enumerate(counting_frames(pkg, d, cam, fl)):
            bad = {c: (got[c], want[c]) for c in COUNTED if got[c] != want[c]}
            assert not bad, (fl, frame, bad)
            assert same(img, product), (fl, frame, n_diff(img, product))


@pytest.mark.parametrize("name", [n for n in S.NAMED if S.NAMED[n][0] == "cubic"])
def test_counters_degree_three(pkg, oracle, name):
    """The counting build with a degree-3 surface (COUNT + HAS_CUBIC) under bfe = 0 / quad_l = 0, by the rules of
    test_counters_fuzz_gpu.test_degree_three_counters: the counting frame is the product frame, the wavefront, no-cull and simple kernels
    book the same five counters, and these lie within that test's bound (cubic_bound: twice what the device's cbrt / acos / cos move the
    oracle's own counters by, at least one flipped pixel's worth) of the oracle under the device's libm."""
    from test_counters_fuzz_gpu import cubic_bound, scene_meta
    osc, cam = build(("named", name))
    d = S.desc(pkg, osc)
    product = render_desc(pkg, d, cam)
    got = counting_frames(pkg, d, cam, 0, n=3)
    for frame, (c, img) in enumerate(got):
        assert same(img, product), (frame, n_diff(img, product))
        assert {k: c[k] for k in COUNTED} == {k: got[0][0][k] for k in COUNTED}, frame
    c = got[0][0]
    for fl in (pkg.RT_FLAG_NOCULL, pkg.RT_FLAG_SIMPLE):
        (other, img), = counting_frames(pkg, d, cam, fl, n=1)
        assert same(img, product), fl
        assert {k: other[k] for k in COUNTED} == {k: c[k] for k in COUNTED}, (fl, other, c)
    plain = osc.render(cam=cam, counters=True, nthreads=8)[1]
    (_, dev), _, _ = D.render_device_libm(D.lib(pkg), osc, cam=cam, counters=True, nthreads=8)
    plain, dev = dict(plain, hits=plain["normals"]), dict(dev, hits=dev["normals"])
    bound = cubic_bound(plain, dev, scene_meta(osc))
    print(f"{name}: plain oracle {[plain[k] for k in COUNTED]} device-libm oracle {[dev[k] for k in COUNTED]} device {[c[k] for k in COUNTED]} "
          f"bound {[bound[k] for k in COUNTED]}")
    for k in COUNTED:
        assert abs(c[k] - dev[k]) <= bound[k], (k, c[k], dev[k], bound[k])


# ---- 3. supersampling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.FAMILIES)
def test_supersampling(pkg, oracle, name):
    """RT_FLAG_SSAA2 / SSAA4, RT_FLAG_SSAA_ADAPTIVE and RT_FLAG_SSAA_GEOMETRY against the composers of the supersampling tests
    (ssaa_ref.resolve, ssaa_adaptive_ref.compose, ssaa_geometry_ref.compose), fed with the oracle's frames.  (A NaN background: the
    adaptive contrast test compares NaN channels.)  RGBA8 frames are held to rgba8_of(composer output), not to ssaa_ref.quantise:
    quantise states no rule for channels outside [0, 1], rgba8_of is the same expression with the low byte taken.  A NaN or inf
    channel of a resolved pixel has no RGBA8 expectation here."""
    osc, _, cams = S.named(name)
    cam = cams[1]
    d = S.desc(pkg, osc)
    p = osc.render(cam=cam, nthreads=8)
    g = gbuffer_ref.compose(osc, cam)

    def check(got, want, what):
        if got.dtype == np.uint8:
            want8, ok = rgba8_of(want)
            assert np.all(got[..., 3] == 255) and not ((got[..., :3] != want8[..., :3]) & ok).any(), what
        else:
            assert same_as_oracle(got, want), what
    for k in (2, 4):
        s = osc.with_size(k * osc.width, k * osc.height).render(cam=cam, nthreads=8)
        kf = {2: pkg.RT_FLAG_SSAA2, 4: pkg.RT_FLAG_SSAA4}[k]
        for fmt in (F32, U8):
            check(render_desc(pkg, d, cam, flags=kf, fmt=fmt), ssaa_ref.resolve(s, k), (name, k, fmt, "resolve"))
            for flags, taus, coses in ((kf | pkg.RT_FLAG_SSAA_ADAPTIVE, (-1.0, 1.0 / 32.0, float("inf")), (None,)),
                                       (kf | pkg.RT_FLAG_SSAA_ADAPTIVE | pkg.RT_FLAG_SSAA_GEOMETRY, (1.0 / 32.0, float("inf")), (-float("inf"), 0.999))):
                r = pkg.Renderer(d, device=0, flags=flags, fmt=fmt)
                try:
                    for tau in taus:
                        for c in coses:
                            r.set_ssaa_threshold(tau)
                            if c is not None:
                                r.set_ssaa_geometry(c)
                            r.update(cam)
                            got, n = r.download(), r.refined
                            if c is None:
                                want, mask = ada.compose(p, s, k, tau), ada.refine_mask(p, tau)
                            else:
                                want = geo.compose(p, s, k, tau, g["object"], g["normal"], c)
                                mask = ada.refine_mask(p, tau) | geo.geo_mask(g["object"], g["normal"], c)
                            assert n == int(mask.sum()), (name, k, fmt, tau, c, n, int(mask.sum()))
                            check(got, want, (name, k, fmt, tau, c))
                finally:
                    r.cleanup_update()


# ---- 4. transport --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F32, U8], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("name", S.FAMILIES)
def test_transport(pkg, name, fmt):
    """Bands of three ranks gathered and put together by rt_assemble, and sparse transport (rt_render_sparse + rt_assemble_sparse):
    the dense single-context frame, bit for bit.  Backgrounds that are negative, -0.0 or NaN: a tile without content is not sent and
    the root repaints it -- to the same bits."""
    import torch
    osc, _, cams = S.named(name)
    cam = cams[0]
    d = S.desc(pkg, osc)
    w, h, world, band = osc.width, osc.height, 3, 8
    want = render_desc(pkg, d, cam, fmt=fmt)
    tdt = torch.uint8 if fmt == U8 else torch.float32
    rs = [pkg.Renderer(d, device=0, rank=r, world=world, band_rows=band, fmt=fmt) for r in range(world)]
    try:
        gathered = torch.zeros((world, rs[0].max_local_rows, w, 4), dtype=tdt, device="cuda:0")
        for r, ren in enumerate(rs):
            ren.update(cam, dev_fb=gathered[r].data_ptr())
        out = torch.zeros((h, w, 4), dtype=tdt, device="cuda:0")
        rs[0].assemble(gathered.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), want), "banded frame"
        cap = max(((w + 15) // 16) * ((ren.local_rows + 15) // 16) for ren in rs)
        nbytes = rs[0].sparse_msg_bytes(cap)
        sent = 0
        for frame in range(3):
            msgs = torch.full((world, nbytes), 0xCD, dtype=torch.uint8, device="cuda:0")
            for r, ren in enumerate(rs):
                ren.update_sparse(msgs[r].data_ptr(), cap, cam)
            out = torch.full((h, w, 4), 9, dtype=tdt, device="cuda:0")
            rs[0].assemble_sparse(msgs.data_ptr(), cap, out.data_ptr())
            torch.cuda.synchronize()
            hdr = msgs.cpu().numpy().view(np.uint32)[:, :2]
            assert not hdr[:, 1].any(), "overflow at full capacity"
            sent = int(hdr[:, 0].sum())
            assert same(out.cpu().numpy(), want), ("sparse frame", frame, n_diff(out.cpu().numpy(), want))
        assert 0 < sent <= sum(((w + 15) // 16) * ((ren.local_rows + 15) // 16) for ren in rs)
    finally:
        for ren in rs:
            ren.cleanup_update()


# ---- 5. RGBA8 of the shipped scenes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quadratic", "20spheres", "reflection_test"])
def test_rgba8_of_the_shipped_scenes_exactly(pkg, name, monkeypatch):
    """The shipped degree <= 2 scenes, every kernel variant: RGBA8 is the stated rounding of the same variant's RGBA32F frame."""
    sc = pkg.Scene.load_from_file(scene_path(name)).set_size(320, 240)
    todo = [("default", 0), ("nocull", pkg.RT_FLAG_NOCULL), ("simple", pkg.RT_FLAG_SIMPLE), ("nolean", pkg.RT_FLAG_NOLEAN)]
    first = None
    for lean in (False, True):
        if lean:
            if name != "20spheres":
                break
            monkeypatch.setenv("MI355RT_LEAN", "always")
            todo = [("lean", 0)]
        for n, fl in todo:
            v = render_desc(pkg, sc, flags=fl)
            q = render_desc(pkg, sc, flags=fl, fmt=pkg.RT_FMT_RGBA8)
            check_rgba8(q, v, f"{name} {n}")
            first = q if first is None else first
            assert np.array_equal(q, first), (name, n)
