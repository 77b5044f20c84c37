"""Full-size parity of BASELINE configs 3, 4 and 5 on one GPU (config 2 is tests/test_gpu_parity.py::test_full_size_properties).

The oracle cannot render these sizes in seconds (config 5 takes a minute on all cores), so the checks are: device work
counters and the frame checksum against tests/golden/survey_anchors.json (SURVEY.md section 8 work table), determinism,
a sample of rows against the oracle (bit-identical for degree <= 2, 1e-5 for the cubic), and -- for the sharded path --
a world = 8, band = 16 render on one GPU whose reassembly equals the single-context frame bit for bit.
"""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cubic_device_lab as D  # noqa: E402  (the oracle under the device's cbrt / acos / cos)

pytestmark = pytest.mark.gpu

A = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "survey_anchors.json")))
CFG = {c["id"]: c for c in A["configs"]}


def _checksum(img):
    """Sum of all RGB channels accumulated in double, row by row (keeps the temporary small at 8K)."""
    s = 0.0
    for y0 in range(0, img.shape[0], 256):
        s += float(img[y0:y0 + 256, :, :3].astype(np.float64).sum())
    return s


def _render(pkg, cfg, **kw):
    sc = pkg.Scene.load_from_file(scene_path(cfg["scene"])).set_size(cfg["w"], cfg["h"])
    if cfg["max_reflections"] is not None:
        sc.set_max_reflections(cfg["max_reflections"])
    r = pkg.Renderer(sc, device=0, **kw)
    r.update()
    img = r.download()
    cnt = r.counters() if kw.get("flags", 0) & pkg.RT_FLAG_COUNT else None
    r.cleanup_update()
    return sc, img, cnt


def _oracle_rows(oracle, cfg, rows):
    s = oracle.load_scene(scene_path(cfg["scene"])).with_size(cfg["w"], cfg["h"], cfg["max_reflections"])
    return s.render(rows=np.asarray(rows, dtype=np.uint32), nthreads=os.cpu_count() or 8)


def test_config3_reflection_test_full_size(pkg, oracle):
    cfg = CFG[3]
    _, a, cnt = _render(pkg, cfg, flags=pkg.RT_FLAG_COUNT)
    _, b, _ = _render(pkg, cfg)
    assert np.array_equal(a, b)
    assert cnt["rays_total"] == cfg["rays"] == 4168418 and cnt["tests"] == cfg["tests"] == 8330054
    assert cnt["reflect_rays"] == cfg["reflect"] and cnt["shadow_rays"] == cfg["shadow"]
    assert abs(_checksum(a) - cfg["checksum"]) < 6e-3
    rows = np.arange(0, cfg["h"], 41)
    assert np.array_equal(a[rows][..., :3], _oracle_rows(oracle, cfg, rows))
    px = [p for p in A["sample_pixels"] if p["config"] == 3][0]
    assert np.allclose(a[px["y"], px["x"], :3], np.array(px["rgb"], dtype=np.float32), rtol=3e-8, atol=1e-9)


def test_config4_clebsch_full_size(pkg, oracle):
    cfg = CFG[4]
    _, a, cnt = _render(pkg, cfg, flags=pkg.RT_FLAG_COUNT)
    _, b, _ = _render(pkg, cfg)
    assert np.array_equal(a, b)
    assert cnt["rays_total"] == cfg["rays"] == 54627972
    # degree-3 surface: device cbrt / acos / cos differ from glibc in the last ulp -> 1e-5 relative per channel, with the
    # flip bound of tests/test_gpu_parity.py::test_cubic_scenes_within_tolerance (<= 0.04 % of the pixels)
    rows = np.arange(180, cfg["h"], 360)   # 6 rows
    assert len(rows) == 6
    c = compare(a[rows][..., :3], _oracle_rows(oracle, cfg, rows))
    assert c["n_bad_pixels"] <= max(2, int(0.0004 * len(rows) * cfg["w"])), c
    # ... and against the oracle under the device's cbrt / acos / cos (tests/tools/cubic_device_lab.py): none beyond 1e-5
    s = oracle.load_scene(scene_path(cfg["scene"])).with_size(cfg["w"], cfg["h"], cfg["max_reflections"])
    c = D.compare_device_libm(pkg, a[rows][..., :3], s, rows=np.asarray(rows, dtype=np.uint32), nthreads=16)
    assert c["n_bad_pixels"] == 0, c
    # the checksum of SURVEY's table: last-ulp differences of the special functions move a channel by ~1e-7 relative (random
    # sign over 25 M channels) and a pixel that flips at a solver discontinuity by < 1; 5.0 of 5.0e6 allows a handful
    d = abs(_checksum(a) - cfg["checksum"])
    assert d < 5.0, d


def test_config5_20spheres_8k_full_size(pkg, oracle):
    cfg = CFG[5]
    _, a, cnt = _render(pkg, cfg, flags=pkg.RT_FLAG_COUNT)
    assert cnt["rays_total"] == cfg["rays"] == 108064010 and cnt["tests"] == cfg["tests"] == 1939852539
    assert abs(_checksum(a) - cfg["checksum"]) < 0.05   # the anchor is printed with 2 decimals; 10^8 float channels
    rows = np.arange(17, cfg["h"], 173)    # 25 rows
    assert np.array_equal(a[rows][..., :3], _oracle_rows(oracle, cfg, rows))
    _, b, _ = _render(pkg, cfg)
    assert np.array_equal(a, b)


def test_4k_world8_band16_reassembles_bit_identical(pkg):
    """BASELINE config 5's partitioning (8 owners, bands of 16 rows) at 3840x2160, the eight contexts on one GPU: every
    rank's rows, gathered rank-major and reassembled by rt_assemble, equal the single-context frame bit for bit."""
    import torch
    w, h, world, band = 3840, 2160, 8, 16
    sc = pkg.Scene.load_from_file(scene_path("20spheres")).set_size(w, h)
    full = pkg.Renderer(sc, device=0)
    full.update()
    want = full.download()
    full.cleanup_update()
    rs = [pkg.Renderer(sc, device=0, rank=r, world=world, band_rows=band) for r in range(world)]
    mx = rs[0].max_local_rows
    gathered = torch.zeros((world, mx, w, 4), dtype=torch.float32, device="cuda:0")
    for r, ren in enumerate(rs):
        assert np.array_equal(ren.row_map(), pkg.band_rows_of_rank(h, band, world, r))
        for _ in range(2):   # second frame: launch-order feedback active
            ren.update(dev_fb=gathered[r].data_ptr())
    out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    rs[0].assemble(gathered.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    for ren in rs:
        ren.cleanup_update()
