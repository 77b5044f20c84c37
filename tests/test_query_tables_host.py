"""The conditions that keep tests/test_query_tables_gpu.py from being vacuous, asserted on the CPU composers alone (tests/tools/rays_ref.py,
gbuffer_ref.py and the oracle) for the very scenes, seeds, target lists, aimed rays and rows that file uses: both take them from
tests/tools/query_table_scenes.py and from nowhere else, so the two files move together.  No GPU and no product kernel runs here."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gbuffer_ref  # noqa: E402
import query_table_scenes as Q  # noqa: E402
import rays_ref  # noqa: E402
import stream_scenes as S  # noqa: E402


def owned(case):
    """The targets whose aimed ray has them as closest hit."""
    hits = rays_ref.closest(case.osc, case.rays)
    return {k for k, got in zip(case.targets, hits["object"].tolist()) if got == k}, hits


def check_aimed_rays_own_their_targets(case, singles=()):
    mine, hits = owned(case)
    assert 3 * len(mine) >= len(case.targets), (len(mine), len(case.targets))
    assert (hits["object"] < 0).any() or not np.isfinite(case.rays["d"]).all(axis=1).all()   # (the odd kinds are there)
    for name, table in Q.tables(case.coefs).items():
        for at, ch in enumerate(Q.chunks(table)):
            assert mine & set(ch), (name, "chunk", at)
    for k in singles:
        assert k in mine, k
    return mine


def check_occlusion_spans_the_chunks(case, at_least, each_pass=True, last_each_pass=True):
    """Blocked and unblocked rays under both t_max choices; under each of them (planes, which cross each other everywhere and which the
    kernels do not take in chunks: under the two together) the lowest-index blocker lies in `at_least` different chunks and in the
    last chunk of a table at least once (the large fields, where a ray without an end meets a sphere of a low index somewhere: under the
    t_max array)."""
    pos = Q.position(case.coefs)
    last = {name: (len(table) - 1) // Q.CHUNK for name, table in Q.tables(case.coefs).items() if table}
    where = set()
    for t_max in (case.t_max, None):
        first = Q.lowest_blocker(case.osc, case.rays, t_max)
        assert np.array_equal(first >= 0, rays_ref.occluded(case.osc, case.rays, t_max) == 1)
        assert (first >= 0).any() and (first < 0).any()
        where = {pos[k] for k in first[first >= 0].tolist()} | (set() if each_pass else where)
        if each_pass or t_max is None:
            assert len(where) >= at_least, where
            assert any(ch == last[name] for name, ch in where) or not (last_each_pass or t_max is not None), where
    assert not np.array_equal(Q.lowest_blocker(case.osc, case.rays, case.t_max), Q.lowest_blocker(case.osc, case.rays))   # (t_max decides somewhere)
    tm = case.t_max
    assert np.isnan(tm).any() and np.isposinf(tm).any() and (tm == Q.K_MAX_T).sum() > len(tm) // 3 and (tm < Q.K_MAX_T).sum() > len(tm) // 4


def last_chunks(coefs):
    return {name: Q.chunks(table)[-1] for name, table in Q.tables(coefs).items() if table}


# ---- a. the small cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Q.SMALL, ids=lambda c: f"{c[1]} {c[0]}")
def test_small_cases(pkg, case):
    kind, n = case
    c = Q.small_case(pkg, case)
    assert c.targets == list(range(n)) and len(c.rays) == n
    refl = np.asarray(c.osc.reflection)
    assert (refl > 0).sum() >= n // 4 and (refl == 0).sum() >= n // 2   # mirrors for the paths, plain surfaces for their ends
    table = Q.tables(c.coefs)
    assert [len(v) for v in table.values() if v] == [n] and table["plane" if kind == "planes" else kind]
    check_aimed_rays_own_their_targets(c, singles=[n - 1] if n % Q.CHUNK == 1 else [])
    check_occlusion_spans_the_chunks(c, at_least=3 if n == 193 else (n - 1) // Q.CHUNK + 1, each_pass=kind != "planes")
    # primary rays: an object of the last chunk owns a pixel of each frame used
    for w, h in Q.SIZES:
        ow = S.Owners(Q.small_case(pkg, case, w, h).osc)
        lo = ((n - 1) // Q.CHUNK) * Q.CHUNK
        if kind == "planes":
            assert any(ow.owner(x, y) >= lo for y in range(0, h, 3) for x in range(0, w, 3)), (w, h)
        else:
            assert ow.some_owner_in(lo, n) is not None, (w, h)


# ---- b. six degree-3 objects ----------------------------------------------------------------------------------------------------------------
def test_the_cubic_scene_shows_objects_beyond_the_fourth(pkg):
    c = Q.cubic_case(pkg)
    cubic = Q.tables(c.coefs)["cubic"]
    assert len(cubic) == 6 and c.osc.width == 64 and c.osc.height == 48
    late = set(cubic[4:])
    obj = gbuffer_ref.compose(c.osc)["object"]
    assert late & set(np.unique(obj).tolist()), "no pixel shows a degree-3 object beyond RT_CUB_AT_MAX"
    mine, _ = owned(c)
    assert late & mine, "no aimed ray is owned by a degree-3 object beyond RT_CUB_AT_MAX"


# ---- c. the large cases ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large(name):
    import __graft_entry__ as graft
    return Q.large_case(graft.load_package(), name)


def test_the_large_cases_are_the_sizes_they_claim(pkg):
    n = S.first_count_beyond_lds(pkg)
    sizes = {name: {k: len(v) for k, v in Q.tables(large(name).coefs).items()} for name in Q.LARGE}
    assert sizes[Q.LARGE[0]] == dict(sphere=n - 1, quadric=0, plane=0, cubic=0)
    assert sizes[Q.LARGE[1]] == dict(sphere=n + 1, quadric=0, plane=0, cubic=0)
    assert sizes[Q.LARGE[2]] == dict(sphere=1000, quadric=1000, plane=2, cubic=0)
    assert sizes[Q.LARGE[3]] == dict(sphere=Q.QUERY_LIMIT_SPHERES, quadric=0, plane=0, cubic=0) and Q.QUERY_LIMIT_SPHERES * 64 == S.LDS_LIMIT == 163840
    assert (np.asarray(large(Q.LARGE[3]).osc.reflection) > 0).sum() > 800 and large(Q.LARGE[3]).osc.max_reflections == 2


@pytest.mark.parametrize("name", Q.LARGE)
def test_large_cases(pkg, name):
    c = large(name)
    n = len(c.coefs)
    assert 150 < len(c.targets) <= 250 + 2 * sum(len(Q.chunks(t)) for t in Q.tables(c.coefs).values()) and set(Q.boundary_targets(c.coefs)) <= set(c.targets)
    singles = [n - 1] if name == Q.LARGE[1] else []   # the large sphere appended last
    check_aimed_rays_own_their_targets(c, singles)
    check_occlusion_spans_the_chunks(c, at_least=10, last_each_pass=False)
    # primary rays: an object of the last chunk of each table owns a pixel of the rows the planes are composed for
    obj = set(np.unique(gbuffer_ref.compose(c.osc, rows=Q.ROWS)["object"]).tolist())
    for table, ch in last_chunks(c.coefs).items():
        assert obj & set(ch), (table, "the last chunk owns no pixel of the composed rows")
    assert all(y0 in Q.ROWS and y1 in Q.ROWS and all(y in Q.ROWS for y in range(y0, y1 + 1)) for _, y0, _, y1 in Q.RECTS_LARGE)


def test_the_moved_case(pkg):
    sc, coefs, c = Q.moved_case(pkg)
    before = large(Q.LARGE[1])
    assert c.targets == before.targets and (np.abs(c.coefs - before.coefs).max(axis=1) > 0).all()
    check_aimed_rays_own_their_targets(c, [len(coefs) - 1])
    # the moved scene answers differently: the aimed rays of the moved scene on the scene before the move
    assert not rays_ref.same_records(rays_ref.closest(before.osc, c.rays), rays_ref.closest(c.osc, c.rays))
