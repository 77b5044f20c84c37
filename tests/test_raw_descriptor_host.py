"""Host checks of tests/tools/raw_desc_scenes.py, the scenes tests/test_raw_descriptor_gpu.py renders: every odd scene differs from
its twin in the oracle's frames (a kernel that treated the odd input as an ordinary one would fail the GPU comparison), and the named
list reaches every arm rt_create's flags select -- backface_exact x quadratic-branch per directional light in every scene class, and
lights_plain cleared by exactly one light."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import raw_desc_scenes as S  # noqa: E402


@pytest.mark.parametrize("name", list(S.NAMED))
def test_odd_scene_differs_from_its_twin(name):
    s, twin, cams = S.named(name)
    assert S.scene_class(s) == S.scene_class(twin) == S.NAMED[name][0]
    assert np.all(np.isfinite(twin.albedo)) and np.all(np.isfinite(twin.light_color)) and S.flags(twin)[2] == 1, "the twin is not ordinary"
    for cam in cams:
        a, b = s.render(cam=cam, nthreads=4), twin.render(cam=cam, nthreads=4)
        n = int((S.bits(a) != S.bits(b)).any(axis=-1).sum())
        assert n >= 10, f"{name}: the oddity changes {n} pixels of the oracle's frame"


def test_named_scenes_reach_every_arm():
    """(bfe, quad_l) of a directional light picks the arm of the general light loop (rt_wavefront.hip, lean path and phase B), and
    n_us <= 64 the lay-out within it: all four combinations in each class; lights_plain = 0 moves the whole launch of a lean scene
    from the specialised loop to the general one, also when one light among forty is the only odd one."""
    seen = {cls: set() for cls in S.CLASSES}
    one_odd_of_many = {cls: 0 for cls in S.CLASSES}
    plain = {cls: set() for cls in S.CLASSES}
    for name in S.NAMED:
        s, _, _ = S.named(name)
        cls = S.scene_class(s)
        bfe, quad, lights_plain, odd = S.flags(s)
        sph = s.light_is_spherical.astype(bool)
        seen[cls] |= {(int(bfe[i]), int(quad[i])) for i in range(len(sph)) if not sph[i]}
        plain[cls].add(lights_plain)
        if len(odd) == 1 and len(sph) > 32 and odd[0] >= 32:
            assert lights_plain == 0
            one_odd_of_many[cls] += 1
    for cls in S.CLASSES:
        assert seen[cls] == {(0, 0), (0, 1), (1, 0), (1, 1)}, (cls, seen[cls])
        assert plain[cls] == {0, 1}, cls
    assert all(one_odd_of_many[cls] >= 1 for cls in ("lean", "lean65", "gq", "mirror")), one_odd_of_many


def test_direction_lengths_at_the_threshold():
    """The two lengths next to sqrt(EPS) are one float apart and fall on either side of rt_create's test after the round trip."""
    a, b = S.at_eps(S.D_T, True), S.at_eps(S.D_T, False)
    assert S.u2_of(a) > S.EPS >= S.u2_of(b)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.array_equal(b.astype(np.float32).astype(np.float64), b)
    k = int(np.argmax(np.abs(a)))
    assert np.nextafter(np.float32(a[k]), np.float32(0)) == np.float32(b[k]) and np.array_equal(np.delete(a, k), np.delete(b, k))


def test_generator_covers_the_classes_and_flags():
    classes, combos, plain = set(), set(), set()
    for seed in range(S.N_SEEDS):
        s, _ = S.scene(seed)
        classes.add(S.scene_class(s))
        bfe, quad, lights_plain, _ = S.flags(s)
        sph = s.light_is_spherical.astype(bool)
        combos |= {(int(bfe[i]), int(quad[i])) for i in range(len(sph)) if not sph[i]}
        plain.add(lights_plain)
    assert classes >= {"lean", "lean65", "gq"} and combos == {(0, 0), (0, 1), (1, 0), (1, 1)} and plain == {0, 1}
