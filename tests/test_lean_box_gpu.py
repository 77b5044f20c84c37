"""The bounding box of a block's (lean schedule) or a chunk's (general schedule) hit points feeds the culling of shadow tests: a box that
misses one lane's hit point culls the occluder that shadows only that point, and the pixel comes out lit.  The scenes here make that
visible: tiny spheres, each seen by exactly one chosen pixel of an 8x8 block (lane = 8 * row + column; a DPP row is two pixel rows), and per
block one large sphere far away towards the light whose shadow falls on exactly one of them -- far outside the margin of the culling
from every other hit of the block.  Frames of both schedules must equal the oracle and a render without culling bit for bit; that the
chosen pixels are the only hits, that the targets are shadowed and that the far spheres are what shadows them is checked with the
oracle first (on the CPU)."""
import functools

import numpy as np
import pytest

from test_gpu_parity import oracle_from, render_desc

pytestmark = pytest.mark.gpu

FOV = 60.0
DEPTH = 20.0
BG = (0.2, 0.3, 0.4)
TO_LIGHT = np.array([0.0, 0.8, -0.6])   # up and back past the camera: the far spheres stand behind the camera, out of every primary ray's way
FAR = 50.0                              # distance of a far sphere from the hit it shadows
FAR_RADIUS = 0.6                        # its radius in pixel spacings at DEPTH: its shadow covers the tiny sphere (0.25) and stays clear of the neighbouring pixels' hits

ROWS = [(1, 0), (6, 2), (3, 5), (4, 7)]        # one pixel in each DPP row (lanes 1, 22, 43, 60)
CORNERS = [(0, 0), (7, 7)]                      # lanes 0 and 63
# (block x, block y, pixels of the block (column, row), index of the pixel that a far sphere shadows)
BLOCKS_64 = [(0, 0, [(0, 0)], 0), (3, 0, [(7, 7)], 0), (6, 1, CORNERS, 0), (1, 2, CORNERS, 1),
             (0, 4, ROWS, 0), (3, 4, ROWS, 1), (6, 4, ROWS, 2), (1, 6, ROWS, 3), (4, 7, [(0, 0), (7, 0), (0, 7), (7, 7)], 2), (7, 6, [(3, 3), (4, 4)], 1)]
# 40 x 24: two and a half tiles by one and a half -- blocks in the partial column (x = 4) and the partial row (y = 2)
BLOCKS_40 = [(0, 0, CORNERS, 1), (2, 0, ROWS, 2), (4, 0, CORNERS, 0), (1, 2, ROWS, 3), (4, 2, [(7, 7)], 0), (3, 1, ROWS, 0)]
FRAMES = {"64x64": (64, 64, BLOCKS_64), "40x24": (40, 24, BLOCKS_40)}


def pixel_point(w, h, x, y, depth=DEPTH):
    """the point at z = depth on the primary ray of pixel (x, y) of the default camera (origin, looking along +z)"""
    t = np.tan(np.radians(0.5 * FOV))
    return depth * np.array([(2.0 * (x + 0.5) / w - 1.0) * (w / h) * t, (2.0 * (y + 0.5) / h - 1.0) * t, 1.0])


def build(pkg, name, with_far=True):
    """-> scene, hit pixels [(x, y)], target pixels [(x, y)]"""
    w, h, blocks = FRAMES[name]
    s = pkg.Scene.new(w, h, FOV, 1, BG)
    spacing = 2.0 * np.tan(np.radians(0.5 * FOV)) / h * DEPTH
    hits, targets, far = [], [], []
    for bx, by, pixels, target in blocks:
        for i, (lx, ly) in enumerate(pixels):
            x, y = 8 * bx + lx, 8 * by + ly
            assert x < w and y < h
            c = pixel_point(w, h, x, y)
            s.add_object(pkg.surface_make("sphere", c, [0.25 * spacing]), (0.9, 0.8, 0.7))
            hits.append((x, y))
            if i == target:
                targets.append((x, y))
                far.append(c + FAR * TO_LIGHT)
    if with_far:
        for c in far:
            s.add_object(pkg.surface_make("sphere", c, [FAR_RADIUS * spacing]), (0.5, 0.5, 0.5))
    s.add_light("directional", -TO_LIGHT)
    s.add_light("directional", [0.3, -0.2, 1.0])   # a second light that nothing blocks: a shadowed target is not simply black
    return s, hits, targets


@functools.lru_cache(maxsize=None)
def reference(pkg, oracle, name):
    """the oracle's frame, computed once per frame size and shared; checked for sensitivity before anything relies on it"""
    sc, hits, targets = build(pkg, name)
    bare, _, _ = build(pkg, name, with_far=False)
    want = oracle_from(pkg, oracle, sc).render(nthreads=8)
    lit = oracle_from(pkg, oracle, bare).render(nthreads=8)
    h, w = want.shape[:2]
    is_hit = np.any(want != np.array(BG, dtype=np.float32), axis=-1)
    assert sorted(zip(*np.nonzero(is_hit)[::-1])) == sorted(hits), "the chosen pixels are not exactly the hits"
    changed = np.any(want != lit, axis=-1)
    assert sorted(zip(*np.nonzero(changed)[::-1])) == sorted(targets), "the far spheres do not shadow exactly the targets"
    for x, y in targets:   # shadowed from the first light: darker in every channel, and still lit by the second
        assert np.all(want[y, x] < lit[y, x]) and np.all(want[y, x] > 0.0)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("name", list(FRAMES))
def test_scenes_are_sensitive(pkg, oracle, name):
    """(CPU only) exactly the chosen pixels hit, exactly the targets change when the far spheres go, and there are targets in lanes 0 and 63"""
    reference(pkg, oracle, name)
    _, hits, targets = build(pkg, name)
    lanes = {(x % 8) + 8 * (y % 8) for x, y in targets}
    assert {0, 63} <= lanes and len(targets) == len(FRAMES[name][2]) and len(hits) < 64


@pytest.mark.parametrize("schedule", ["lean", "general"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_frames_equal_oracle_and_unculled_render(pkg, oracle, monkeypatch, name, schedule):
    # rt_create reads MI355RT_LEAN: frames as small as these would otherwise leave the lean schedule after the first one
    monkeypatch.setenv("MI355RT_LEAN", "always")
    flags = pkg.RT_FLAG_NOLEAN if schedule == "general" else 0
    want = reference(pkg, oracle, name)
    sc, _, targets = build(pkg, name)
    got = render_desc(pkg, sc, flags=flags)
    plain = render_desc(pkg, sc, flags=flags | pkg.RT_FLAG_NOCULL)
    bad = np.nonzero(np.any(got[..., :3] != want, axis=-1))
    assert bad[0].size == 0, ("differs from the oracle at (x, y)", list(zip(*bad[::-1]))[:8], "targets", targets)
    assert np.array_equal(got, plain), "culling changed pixels"
    # the culling did work in these frames: fewer sphere tests executed than without it
    if schedule == "lean":
        counts = []
        for fl in (flags, flags | pkg.RT_FLAG_NOCULL):
            r = pkg.Renderer(sc, device=0, flags=fl | pkg.RT_FLAG_COUNT)
            r.update()
            counts.append(r.counters()["tests_executed"])
            r.cleanup_update()
        assert counts[0] < counts[1], counts
