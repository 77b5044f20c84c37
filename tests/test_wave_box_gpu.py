"""The box helper of the render kernel run alone (rt_debug_wave_box; csrc/rt_wave_box.hpp): six fused DPP min / max chains over the 64 lanes
of a wave, fed by FP64 -> FP32 conversions rounded towards -inf / +inf.  Everything is compared with numpy on the float bit patterns:
lo = min over the used lanes of the largest float32 <= x, hi = max of the smallest float32 >= x, from np.float32(x) and np.nextafter."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32_MAX = float(np.finfo(np.float32).max)


def round_down(x):
    """largest float32 <= x, elementwise (x float64); NaN stays NaN"""
    with np.errstate(over="ignore", invalid="ignore"):
        f = x.astype(np.float32)
        return np.where(f.astype(np.float64) <= x, f, np.nextafter(f, np.float32(-np.inf))).astype(np.float32)


def round_up(x):
    """smallest float32 >= x"""
    with np.errstate(over="ignore", invalid="ignore"):
        f = x.astype(np.float32)
        return np.where(f.astype(np.float64) >= x, f, np.nextafter(f, np.float32(np.inf))).astype(np.float32)


def expected(pts, masks):
    """[n, 6] float32: lox, hix, loy, hiy, loz, hiz -- fminf / fmaxf over the used lanes (a NaN drops out), (+inf, -inf) for none"""
    n = pts.shape[0]
    used = ((masks[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)   # [n, 64]
    lo = np.where(used[:, :, None], round_down(pts), np.float32(np.inf))
    hi = np.where(used[:, :, None], round_up(pts), np.float32(-np.inf))
    out = np.empty((n, 6), dtype=np.float32)
    out[:, 0::2] = np.fmin.reduce(lo, axis=1, initial=np.float32(np.inf))
    out[:, 1::2] = np.fmax.reduce(hi, axis=1, initial=np.float32(-np.inf))
    return out


def test_the_expectation_itself():
    """round_down / round_up on values whose answers are known without them"""
    one_up = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    x = np.array([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 1e39, -1e39, 1e-50, -1e-50, 0.0, -0.0, np.inf, -np.inf])
    lo, hi = round_down(x), round_up(x)
    tiny = float(np.nextafter(np.float32(0.0), np.float32(1.0)))
    assert lo.tolist() == [1.0, 1.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))), F32_MAX, -np.inf, 0.0, -tiny, 0.0, -0.0, np.inf, -np.inf]
    assert hi.tolist() == [1.0, one_up, 1.0, np.inf, -F32_MAX, tiny, -0.0, 0.0, -0.0, np.inf, -np.inf]
    assert np.signbit(lo[8]) and np.signbit(hi[8]) and not np.signbit(lo[7]) and np.signbit(hi[6])
    assert np.all(lo.astype(np.float64) <= x) and np.all(hi.astype(np.float64) >= x)


ROW = np.uint64(0xFFFF)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def values(rng, kind, shape):
    sign = rng.choice([-1.0, 1.0], size=shape)
    if kind == "mixed":        # mixed sign, magnitudes from 1e-30 to 1e30
        return sign * 10.0 ** rng.uniform(-30, 30, size=shape)
    f = (sign * 10.0 ** rng.uniform(-30, 30, size=shape)).astype(np.float32).astype(np.float64)
    if kind == "float32":      # exactly representable
        return f
    if kind == "ulp_above":    # one double ulp above / below a float32
        return np.nextafter(f, np.inf)
    if kind == "ulp_below":
        return np.nextafter(f, -np.inf)
    if kind == "subnormal":    # float32-subnormal doubles, and doubles below the smallest of them
        return sign * 10.0 ** rng.uniform(-52, -38.5, size=shape)
    if kind == "huge":         # around and above FLT_MAX, both signs, infinities among them
        pick = rng.integers(0, 6, size=shape)
        table = np.array([F32_MAX, np.nextafter(F32_MAX, np.inf), np.nextafter(F32_MAX, 0.0), 1e39, 1e300, np.inf])
        return sign * table[pick]
    if kind == "near":         # a narrow cluster, as a block's hit points are: many lanes share their leading bits
        return 3.0 + rng.uniform(-1e-6, 1e-6, size=shape)
    raise KeyError(kind)


KINDS = ("mixed", "float32", "ulp_above", "ulp_below", "subnormal", "huge", "near")


@pytest.fixture(scope="module")
def cases():
    """(pts [n, 64, 3], masks [n], label per wave): a few hundred waves for one call"""
    rng = np.random.default_rng(20260)
    pts, masks, labels = [], [], []

    def add(p, m, label):
        pts.append(p)
        masks.append(np.uint64(m))
        labels.append(label)
    for lane in range(64):   # each single lane: the other 63 hold values that would win
        add(values(rng, KINDS[lane % 4], (64, 3)), np.uint64(1) << np.uint64(lane), f"lane {lane}")
    for name, m in (("row 0", ROW), ("row 3", ROW << np.uint64(48)), ("rows 0+2", ROW | (ROW << np.uint64(32))), ("rows 1+3", (ROW << np.uint64(16)) | (ROW << np.uint64(48))),
                    ("all", ALL), ("none", np.uint64(0))):
        for kind in KINDS:
            add(values(rng, kind, (64, 3)), m, f"{name}, {kind}")
    for i in range(30 * len(KINDS)):   # random masks of every density
        kind = KINDS[i % len(KINDS)]
        m = rng.integers(0, 1 << 63, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, dtype=np.uint64)
        if i % 3 == 1:
            m &= rng.integers(0, 1 << 63, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, dtype=np.uint64)
        if i % 3 == 2:
            m &= np.uint64(0xF) << np.uint64(4 * (i % 16))   # inside one group of four lanes
        add(values(rng, kind, (64, 3)), m, f"random mask {int(m):#018x}, {kind}")
    # signed zeros: alone in a lane, and a whole wave of one sign (a wave that mixes the two as its extremum has no one answer)
    for z in (0.0, -0.0):
        p = values(rng, "mixed", (64, 3))
        p[17] = z
        add(p, np.uint64(1) << np.uint64(17), f"zero {z!r} in lane 17")
        add(np.full((64, 3), z), ALL, f"all {z!r}")
        q = np.abs(values(rng, "mixed", (64, 3))) * (1.0 if z == 0.0 and not np.signbit(z) else -1.0)
        q[40] = z   # the minimum of non-negative values / the maximum of non-positive ones
        add(q, ALL, f"zero {z!r} as the extremum")
    return np.array(pts), np.array(masks, dtype=np.uint64), labels


@pytest.fixture(scope="module")
def renderer(pkg):
    sc = pkg.Scene.new(16, 16, 60.0, 1, (0.0, 0.0, 0.0))
    sc.add_object(pkg.surface_make("sphere", [0, 0, 5], [1.0]), (1, 1, 1))
    sc.add_light("directional", [0, -1, 0])
    r = pkg.Renderer(sc, device=0)
    yield r
    r.cleanup_update()


def test_box_equals_numpy_bit_for_bit(renderer, cases):
    pts, masks, labels = cases
    assert 300 <= len(masks) <= 600
    got = renderer.wave_box(pts, masks)
    want = expected(pts, masks)
    assert not np.isnan(want).any()
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, [(labels[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    none = [i for i, l in enumerate(labels) if l.startswith("none")]
    assert len(none) == len(KINDS) and np.all(got[none] == np.array([np.inf, -np.inf] * 3, dtype=np.float32))


def test_a_nan_lane_drops_out(renderer):
    """One NaN coordinate among finite ones: the fminf / fmaxf result over the lanes, as the reductions this helper replaced gave it."""
    rng = np.random.default_rng(7)
    pts = values(rng, "mixed", (64, 64, 3))
    for w in range(64):
        pts[w, w, w % 3] = np.nan          # every lane position once
    masks = np.full(64, ALL, dtype=np.uint64)
    masks[9] = np.uint64(1) << np.uint64(9)   # the NaN lane alone
    got = renderer.wave_box(pts, masks)
    want = expected(pts, masks)
    assert not np.isnan(want).any() and want[9, 0] == np.inf and want[9, 1] == -np.inf
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_repeated_calls_and_one_wave(renderer, cases):
    """n_waves = 1, and the same answer on a second call (the rounding mode is restored: a frame rendered in between is the oracle's)"""
    pts, masks, _ = cases
    a = renderer.wave_box(pts[70:71], masks[70:71])
    renderer.update()
    frame = renderer.download().copy()
    b = renderer.wave_box(pts[70:71], masks[70:71])
    renderer.update()
    assert np.array_equal(a.view(np.uint32), expected(pts[70:71], masks[70:71]).view(np.uint32)) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(frame, renderer.download())
