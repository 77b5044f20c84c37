"""The conditions that keep tests/test_cubic_chunks_gpu.py from being vacuous, on the oracle alone (no GPU): the scenes of
tests/tools/cubic_field_scenes.py under the seed used there show degree-3 objects of every 64-entry chunk of their table, and the
objects behind the first chunk matter to pixels they do not own -- through a shadow only they cast and through a bounce that meets
them.  A streamed kernel that dropped, repeated or left early a chunk of the degree-3 index list (csrc/rt_stream.hpp: sq_tables)
therefore changes these frames; so does a staged loop that stops short (rq_tables, S.cub[j]).  The two files move together: change
F.SEED or F.SCENES and both run on the new scenes.  Measured numbers: DESIGN.md section 8."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cubic_field_scenes as F  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import stream_cull_lab as SC  # noqa: E402

BEYOND = [name for name, kw in F.SCENES.items() if kw["n"] > F.CHUNK]


@functools.lru_cache(maxsize=None)
def conditions(name):
    osc = F.scene(name)
    return osc, F.Conditions(osc)


def test_the_recipe():
    """The translation is exact up to rounding (F(x - c) evaluated both ways), the origin lies outside every surface (F > 0 there, the
    sign of the outside of a body), and the table positions are Q.tables' -- no longer object indices once other classes are there."""
    osc = F.scene("65 quadric")
    rng = np.random.default_rng(0)
    q = np.zeros(20)
    q[:10], q[10:16], q[16:19], q[19] = rng.uniform(-1, 1, 10), rng.uniform(-1, 1, 6), rng.uniform(-1, 1, 3), -1.0
    c = np.array([0.7, -1.3, 2.1])
    qt = F.translated(q, c)
    for p in rng.uniform(-3, 3, (20, 3)):
        mono = lambda v: np.array([np.prod(v ** np.array(e)) for e in F.MONOMIALS])
        assert abs(qt @ mono(p) - q @ mono(p - c)) <= 1e-11 * np.abs(qt * mono(p)).sum()
    table = Q.tables(osc.coefs)["cubic"]
    assert len(table) == 65 and len(osc.objects) == 66 and Q.tables(osc.coefs)["quadric"] == [65]
    assert all(osc.coefs[k][19] > 0.0 for k in table)                      # F(0) > 0: the camera is outside
    assert all((osc.coefs[k][[2, 5, 7]] < 0.0).all() and not osc.coefs[k][[0, 1, 3, 4, 6, 8, 9]].any() for k in table)
    assert [o.reflection_ratio for o in osc.objects[:6]] == [0.5, 0.0, 0.0, 0.5, 0.0, 0.0]
    sph = F.scene("65 spheres")
    t = Q.tables(sph.coefs)
    assert len(t["cubic"]) == 65 and len(t["sphere"]) == 65 and not t["quadric"] and not t["plane"]


def test_a_full_chunk_shows_its_last_entry():
    """n = 64: one exactly full chunk, whose last entry owns pixels; so do the first RT_CUB_AT_MAX (the HOST_CUB branch)."""
    _, c = conditions("64")
    assert c.n == 64 and c.some_pixel_owned_in(63, 64) is not None and c.some_pixel_owned_in(0, F.RT_CUB_AT_MAX) is not None


@pytest.mark.parametrize("name", BEYOND)
def test_every_chunk_owns_pixels(name):
    """Some pixel is owned at a table position >= 64 -- for n = 65 that is position 64 itself; for n = 129 one at >= 128 and another
    within 64 .. 127 -- some by the first RT_CUB_AT_MAX positions, some by positions 4 .. 63, and no pixel shows the background."""
    osc, c = conditions(name)
    assert c.some_pixel_owned_in(F.CHUNK, c.n) is not None
    if c.n == 129:
        assert c.some_pixel_owned_in(128, 129) is not None and c.some_pixel_owned_in(64, 128) is not None
    assert c.some_pixel_owned_in(0, F.RT_CUB_AT_MAX) is not None and c.some_pixel_owned_in(F.RT_CUB_AT_MAX, F.CHUNK) is not None
    owners = set(c.owner[c.owner >= 0].tolist())
    print(f"{name}: {len(owners)} of {c.n} degree-3 objects are nearest on some primary ray; {int((c.owner >= F.CHUNK).sum())} pixels at positions >= 64, "
          f"{int((c.owner >= 128).sum())} at >= 128, {int((c.owner < 0).sum())} without a degree-3 hit")
    assert (c.owner >= 0).all() and len(owners) >= c.n - 8


@pytest.mark.parametrize("name", BEYOND)
def test_a_shadow_only_the_later_chunks_cast(name):
    """What an early exit between chunks would break: some primary hit has a shadow ray towards a light that objects at positions
    >= 64 block and no other object does."""
    _, c = conditions(name)
    found = c.shadow_only_beyond(F.CHUNK)
    print(f"{name}: {len(found)} shadow rays blocked only from positions >= 64" + (" (of the 12 candidates tried)" if c.others else ""))
    assert found


@pytest.mark.parametrize("name", BEYOND)
def test_a_bounce_meets_the_later_chunks(name):
    """Some first bounce of a mirror hit has its nearest hit on an object at a position >= 64."""
    _, c = conditions(name)
    found = c.bounce_met_beyond(F.CHUNK)
    print(f"{name}: {len(found)} first bounces meet a position >= 64 first")
    assert found


@pytest.mark.parametrize("name", BEYOND)
def test_removing_the_later_chunks_changes_pixels_they_do_not_own(name):
    """The oracle's frame without the objects at positions >= 64 differs in pixels where none of them is even the nearest degree-3
    object: those change through shadows and bounces alone."""
    osc, c = conditions(name)
    changed = F.changed_pixels(osc, range(F.CHUNK, c.n))
    elsewhere = changed & ~(c.owner >= F.CHUNK)
    print(f"{name}: removing positions >= 64 changes {int(changed.sum())} pixels, {int(elsewhere.sum())} of which they do not own")
    assert elsewhere.any() and (changed & (c.owner >= F.CHUNK)).any()


@pytest.mark.parametrize("name", [n for n in BEYOND if F.SCENES[n].get("spheres")])
def test_the_sphere_field_gives_the_culling_something_to_decide(name):
    """With the 65 spheres the unit-sphere table has two chunks and mirrors: the scene image says RT_FLAG_STREAM_CULL culls, and the
    rule of include/mi355rt.h gives RT_FLAG_STREAM_CULL_BOUNCE its decision too."""
    osc, _ = conditions(name)
    w = SC.image(SC.arrays_of_oracle(osc))[2]
    assert w["cull"] and (w["n_us"] + 63) // 64 >= 2 and w["n_us"] == 65
    assert (osc.reflection.astype(np.float64) > 1e-7).any() and osc.max_reflections >= 1
