"""The scenes beyond the 160 KiB limit of the staged query kernels (tests/test_stream_queries_host.py, tests/test_stream_queries_gpu.py) --
test infrastructure.  All of them are query_table_scenes.Case objects built with the generators that exist (stream_scenes.field,
stream_scenes.mixed_large), so targets, aimed rays and t_max follow the rules of tests/tools/query_table_scenes.py; a context takes them
only with RT_FLAG_STREAM_QUERIES (csrc/rt_stream_queries.hip).

The two test files use the cases and seeds of this module and nothing else: they move together."""
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_table_scenes as Q  # noqa: E402
import stream_scenes as S  # noqa: E402

BEYOND = ["one chunk more", "mirror field", "mixed beyond"]
MIRROR_SPHERES = Q.QUERY_LIMIT_SPHERES + 65   # 2 560 + 65: a full 41st chunk and one entry in the 42nd
MIXED_OBJECTS = 2100                          # 1 050 spheres, 1 050 general quadrics, 2 planes: 168 096 table bytes
MIRROR_SEED = 45                              # a seed under which the conditions of tests/test_stream_queries_host.py hold (the single sphere of the 42nd chunk owns a pixel of Q.ROWS)
FIELD_PREFIXES = (1, 63, 64, 65, 257)         # ray counts around a wave and around a workgroup


def beyond_scene(pkg, name):
    if name == BEYOND[0]:   # 2 561 field spheres and the large one: the 41st chunk holds the last field sphere and the large sphere
        return S.field(pkg, Q.QUERY_LIMIT_SPHERES + 1, S.LARGE_SEED, big_last=True)
    if name == BEYOND[1]:
        return S.field(pkg, MIRROR_SPHERES, MIRROR_SEED, mirrors=True, depth=2)
    assert name == BEYOND[2]   # (the generator has two planes, a floor and a back wall: the plane table stays below one chunk)
    return S.mixed_large(pkg, MIXED_OBJECTS, S.MIXED_SEED)


def beyond_case(pkg, name):
    sc = beyond_scene(pkg, name)
    return Q.Case(sc, S.oracle_of(pkg, sc), False)


@functools.lru_cache(maxsize=None)
def beyond(name):
    """The case, formed once per process and left unchanged."""
    import __graft_entry__ as graft
    return beyond_case(graft.load_package(), name)


def table_bytes(coefs):
    """The class tables' bytes in the scene blob (rt_scene_dev.h: UsEntry 64, GqEntry 96, LinEntry 48, 4 per degree-3 index, each table
    padded to 16)."""
    t = Q.tables(coefs)
    return 64 * len(t["sphere"]) + 96 * len(t["quadric"]) + 48 * len(t["plane"]) + (4 * len(t["cubic"]) + 15) // 16 * 16


def moved_beyond(pkg):
    """BEYOND[0] after every sphere moved (query_table_scenes.moved_coefs): the scene before, the coefficients, the case of the moved scene."""
    sc = beyond_scene(pkg, BEYOND[0])
    coefs = Q.moved_coefs(sc)
    return sc, coefs, Q.Case(Q.with_coefs(pkg, sc, coefs), Q.oracle_with_coefs(S.oracle_of(pkg, sc), coefs), False)
