"""The scene image of csrc/rt_scene_image.hpp against what a context holds on the device, byte for byte.

rt_create uploads what rtp::scene_image returns; the test tools call the same function on the host (tests/tools/scene_pack_lab.py,
whose records tests/test_set_scene_host.py holds to the packing code of old).  Here the two meet: rt_debug_scene_blob of a strict and of
an RT_FLAG_FAST context -- the blob with its class tables, offsets and 16-byte rounding, DevLight[] and LightK[] -- must equal the
host-built image.  One 32x24 scene with an object for every case of the class tables; there is no tolerance."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def scene(pkg):
    def quadric(sq, cross, centre, c):
        q = np.zeros(20)
        q[10:13], q[13:16] = sq, cross
        q[16:19] = -2.0 * np.asarray(sq) * np.asarray(centre)
        q[19] = c
        return q
    plane = np.zeros(20)
    plane[16:20] = (0.05, 1.0, 0.02, 4.0)
    coefs = np.array([quadric((1, 1, 1), (0, 0, 0), (0.0, 0.0, 10.0), 99.0),           # a unit sphere with a bounding radius: r^2 = 100 - 99
                      quadric((1, 1, 1), (0, 0, 0), (1.0, 0.0, 8.0), 70.0),            # unit squares, but r^2 = 65 - 70 < 0: in the sphere table, never culled
                      quadric((1.0, 2.0, 0.5), (0, 0, 0), (3.0, 2.0, 12.0), 150.0),    # an ellipsoid
                      quadric((1.0, 2.0, 0.5), (0.25, 0, 0), (-3.0, 1.0, 12.0), 60.0), # a quadric with a cross term
                      plane,
                      pkg.surface_make("clebsch")])                                     # degree 3
    n = len(coefs)
    albedo = np.linspace(0.1, 0.9, 3 * n, dtype=np.float32).reshape(n, 3)
    reflection = np.array([0.0, 0.5, 0.0, 0.0, 0.0, 0.0], np.float32)
    kinds = np.array([1, 0], np.uint8)                                                   # a point light, and a directional light without a direction
    light_p = np.array([(2.0, 8.0, 2.0), (0.0, 0.0, 0.0)], np.float64)
    light_color = np.array([(300.0, 280.0, 260.0), (0.9, 0.9, 0.8)], np.float32)
    return coefs, reflection, albedo, kinds, light_p, light_color


def test_device_scene_equals_the_host_built_image(pkg):
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import scene_pack_lab as L
    coefs, reflection, albedo, kinds, light_p, light_color = scene(pkg)
    d = pkg.desc_from_arrays(32, 24, float(np.radians(50.0)), np.array([0.1, 0.2, 0.3], np.float32), 2, coefs, reflection, albedo, kinds, light_p, light_color)
    n_lights, blobs = len(kinds), {}
    for flags in (pkg.RT_FLAG_STRICT, pkg.RT_FLAG_FAST):
        want = L.scene_image(coefs, reflection, albedo, kinds, light_p, light_color, flags=flags)
        r = pkg.Renderer(d, device=0, flags=flags)
        try:
            got = r.debug_scene_blob()
        finally:
            r.cleanup_update()
        lights = n_lights * (144 + 128)   # DevLight[] and LightK[] behind the blob (csrc/rt_scene_dev.h)
        assert got.size == want.size and got.size > lights + 6 * 224
        assert np.array_equal(got[:-lights], want[:-lights]), f"flags {flags}: the blob differs, first at byte {int(np.flatnonzero(got[:-lights] != want[:-lights])[0])}"
        assert np.array_equal(got[-lights:], want[-lights:]), f"flags {flags}: the light tables differ"
        blobs[flags] = got
    assert np.array_equal(blobs[pkg.RT_FLAG_STRICT], blobs[pkg.RT_FLAG_FAST])   # the image is the scene's, not the variant's
