"""What tests/test_counters_fuzz_gpu.py assumes about the oracle's counters, pinned on the CPU: they do not depend on the number of
threads, they add up over any partition of the rows (so a band's counters are the oracle's for its rows), every test is booked under
exactly one solver branch, every hit sends one shadow ray per light and at most that many are shaded."""
import numpy as np
import pytest

from test_cubic_gpu import many_cubic_objects_and_mirrors
from test_gpu_parity import mixed_scene, oracle_from, random_cubic_scene, random_scene
from test_oracle_units import two_mirror_scene

BRANCHES = ("br_cardano", "br_trig", "br_quad_hit", "br_quad_miss", "br_linear", "br_none")


def _scenes(pkg, oracle):
    """(name, oracle scene, camera)"""
    out = []
    for seed, n, lights, plane, mirrors in ((1, 4, 1, True, False), (2, 9, 4, False, True), (3, 20, 7, True, True), (4, 40, 3, False, False),
                                            (5, 70, 5, True, True), (6, 33, 2, False, True)):
        cam = pkg.camera_matrix((0.3 * seed - 1.0, 0.5, -4.0), 90.0 + 2 * seed, -3.0 + seed) if seed % 3 else None
        out.append((f"random{seed}", oracle_from(pkg, oracle, random_scene(pkg, 8200 + seed, n, lights, w=160, h=120, with_plane=plane, mirrors=mirrors)), cam))
    for seed in (3, 11, 17):
        out.append((f"mixed{seed}", oracle_from(pkg, oracle, mixed_scene(pkg, seed, 96, 72)), None))
    sc, cam = random_cubic_scene(pkg, 1, 64, 48)
    out.append(("random_cubic1", oracle_from(pkg, oracle, sc), cam))
    out.append(("many_cubic", oracle_from(pkg, oracle, many_cubic_objects_and_mirrors(pkg)).with_size(80, 60), None))
    out.append(("two_mirrors", two_mirror_scene(oracle, 5), None))
    return out


@pytest.fixture(scope="module")
def scenes(pkg, oracle):
    return _scenes(pkg, oracle)


def test_counters_do_not_depend_on_the_thread_count(scenes):
    for name, osc, cam in scenes:
        a, b = osc.render(cam=cam, counters=True, nthreads=1)[1], osc.render(cam=cam, counters=True, nthreads=8)[1]
        assert a == b, name


@pytest.mark.parametrize("world,band", [(2, 1), (3, 5), (4, 3), (5, 8), (8, 16), (2, 33)])
def test_counters_add_up_over_band_cyclic_rows(pkg, scenes, world, band):
    for name, osc, cam in scenes:
        full = osc.render(cam=cam, counters=True, nthreads=4)[1]
        total = dict.fromkeys(full, 0)
        seen = np.zeros(osc.height, dtype=bool)
        for rank in range(world):
            rows = pkg.band_rows_of_rank(osc.height, band, world, rank)
            if len(rows) == 0:
                continue
            part = osc.render(cam=cam, rows=rows, counters=True, nthreads=4)[1]
            seen[rows] = True
            for k in total:
                total[k] += part[k]
        assert seen.all() and total == full, (name, {k: (total[k], full[k]) for k in full if total[k] != full[k]})


def test_relations_between_the_oracles_counters(scenes):
    for name, osc, cam in scenes:
        c = osc.render(cam=cam, counters=True, nthreads=4)[1]
        n_lights = len(osc.lights)
        assert sum(c[b] for b in BRANCHES) == c["tests"], (name, c)
        assert c["shadow_rays"] == c["normals"] * n_lights, (name, c)
        assert c["surface_colors"] <= c["shadow_rays"], (name, c)
        assert c["primary_rays"] == osc.width * osc.height, (name, c)
        assert c["rays_total"] == c["primary_rays"] + c["shadow_rays"] + c["reflect_rays"]
