#!/usr/bin/env python3
"""CPU lab behind the culling and skip predicates of rt_wavefront_math.hpp (tests/tools/cull_lab.cpp: the kernels' own header compiled
for the host, the oracle as the truth).  Two sources of input: every block, tile and chunk of real frames (`frame_sources`), and a
grazing generator that places a sphere tangent -- at relative clearances +-1e-1 ... +-1e-15 -- to a ray of a block, an edge ray of a
tile, or a shadow ray of a chunk (`graze_primary`, `graze_shadow`).  No GPU.
usage: python tests/tools/cull_lab.py [n] [first_seed]      n grazing cases per predicate family (default 200000)"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as graft  # noqa: E402

O = graft.load_oracle()
O.build()

EPS, MAX_T = 1e-7, 1e6
REC = {"cone": 12, "pyr": 21, "sh": 26, "us": 5, "gq": 4}
GP_W, GS_W = 26, 10 + 6 * 64
KINDS = ("cone", "pyr", "sh", "us", "gq")
# the properties, by the name the tables print
PREDICATES = ("us_needs_solve", "needs_solve", "sphere_in_cone", "sphere_in_pyramid", "sphere_relevant<false>", "sphere_relevant<true>",
              "crec_relevant", "crec_in_box_shadow")


class Out(C.Structure):
    _fields_ = [("rec", C.POINTER(C.c_double)), ("truth", C.POINTER(C.c_int32)), ("cap", C.c_uint64), ("n", C.c_uint64)]


class LabOut(C.Structure):
    _fields_ = [(k, Out) for k in KINDS] + [("corner_n", C.c_uint64), ("corner_bad", C.c_uint64), ("corner_worst", C.c_double)] + \
               [(k, C.c_uint64) for k in ("own_n", "own_skip", "own_bad", "bf_n", "bf_skip", "bf_bad", "bf_negzero")]


_LIB = None


def build():
    global _LIB
    if _LIB is not None:
        return _LIB
    out = os.path.join(ROOT, "tests", "tools", "bin", "libcull_lab.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tools", "flopcount_shim"),
                    "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "cull_lab.cpp"), "-o", out,
                    "-L" + os.path.join(ROOT, "oracle"), "-lrt_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle")], check=True)
    lib = C.CDLL(out)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.lab_frame.argtypes = [C.c_void_p, dp, C.POINTER(LabOut), C.c_int]
    lib.lab_graze_primary.argtypes = [C.c_uint64, dp, C.POINTER(LabOut), dp]
    lib.lab_graze_shadow.argtypes = [C.c_uint64, dp, C.POINTER(LabOut), dp]
    for k in ("cone", "pyr", "us", "gq"):
        getattr(lib, "lab_eval_" + k).argtypes = [C.c_uint64, dp, ip]
    lib.lab_eval_sh.argtypes = [C.c_uint64, dp, ip, dp]
    lib.lab_oracle_root.restype = C.c_double
    lib.lab_oracle_root.argtypes = [dp, dp, dp]
    _LIB = lib
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Records:
    """What a generator produced: per kind the records [n, width] and the oracle's verdict [n] (1: some ray of the set accepts), and the
    counters of the properties that need no record (corner claim, own-sphere window, backface skips)."""

    def __init__(self, caps):
        self.buf = {k: (np.zeros((max(1, caps.get(k, 0)), REC[k])), np.zeros(max(1, caps.get(k, 0)), dtype=np.int32)) for k in KINDS}
        self.out = LabOut()
        for k in KINDS:
            o = getattr(self.out, k)
            o.rec, o.truth = _dp(self.buf[k][0]), self.buf[k][1].ctypes.data_as(C.POINTER(C.c_int32))
            o.cap, o.n = caps.get(k, 0), 0
        self.out.corner_worst = np.inf

    def get(self, k):
        o = getattr(self.out, k)
        assert o.n <= o.cap, f"{k}: {o.n} records for a buffer of {o.cap}"
        return self.buf[k][0][:o.n], self.buf[k][1][:o.n]

    def counters(self):
        return {k: getattr(self.out, k) for k in ("corner_n", "corner_bad", "corner_worst", "own_n", "own_skip", "own_bad", "bf_n", "bf_skip", "bf_bad", "bf_negzero")}


def evaluate(kind, rec):
    """The predicates on records: int32 verdicts (and, for "sh", the cull_record fields [n, 6])."""
    lib = build()
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, REC[kind])
    v = np.zeros(len(rec), dtype=np.int32)
    vp = v.ctypes.data_as(C.POINTER(C.c_int32))
    if kind == "sh":
        crec = np.zeros((len(rec), 6))
        lib.lab_eval_sh(len(rec), _dp(rec), vp, _dp(crec))
        return v, crec
    getattr(lib, "lab_eval_" + kind)(len(rec), _dp(rec), vp)
    return v


def frame(osc, cam=None, caps=None, stride=1):
    """Every block, tile and chunk of one frame of an oracle scene."""
    lib = build()
    n_px, n_o, n_l = osc.width * osc.height, max(1, len(osc.objects)), max(1, len(osc.lights))
    blocks = ((osc.width + 7) // 8) * ((osc.height + 7) // 8)
    caps = caps or {"cone": blocks * n_o, "pyr": blocks * n_o, "sh": (2 * blocks + n_px // 64 + 8) * n_o * n_l,
                    "us": (n_px // stride + 64) * n_o * (1 + n_l), "gq": (n_px // stride + 64) * n_o}
    r = Records(caps)
    sc = osc.c_scene()
    cam = np.ascontiguousarray(O.IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
    lib.lab_frame(C.byref(sc), _dp(cam), C.byref(r.out), int(stride))
    return r


# ---- verdicts against the truth ------------------------------------------------------------------------------------------------
class Tally:
    """Per predicate: evaluations, culled (answered "skip"), unsound (skipped although the oracle accepts), and the three equalities."""

    def __init__(self):
        self.n = {p: 0 for p in PREDICATES}
        self.culled = {p: 0 for p in PREDICATES}
        self.unsound = {p: 0 for p in PREDICATES}
        self.accepts = {p: 0 for p in PREDICATES}
        self.crec_differs = self.box_overloads_differ = self.nonfinite_culled = 0
        self.examples = []
        self.c = {"corner_n": 0, "corner_bad": 0, "corner_worst": np.inf, "own_n": 0, "own_skip": 0, "own_bad": 0, "bf_n": 0, "bf_skip": 0, "bf_bad": 0, "bf_negzero": 0}

    def _add(self, name, verdict, truth, rec):
        self.n[name] += len(verdict)
        self.culled[name] += int((verdict == 0).sum())
        self.accepts[name] += int((truth != 0).sum())
        bad = (verdict == 0) & (truth != 0)
        self.unsound[name] += int(bad.sum())
        for i in np.flatnonzero(bad)[:3]:
            self.examples.append((name, rec[i].copy()))

    def add(self, r):
        rec, truth = r.get("us")
        if len(rec):
            self._add("us_needs_solve", evaluate("us", rec), truth, rec)
        rec, truth = r.get("gq")
        if len(rec):
            self._add("needs_solve", evaluate("gq", rec), truth, rec)
        rec, truth = r.get("cone")
        if len(rec):
            self._add("sphere_in_cone", evaluate("cone", rec), truth, rec)
        rec, truth = r.get("pyr")
        if len(rec):
            self._add("sphere_in_pyramid", evaluate("pyr", rec), truth, rec)
        rec, truth = r.get("sh")
        if len(rec):
            self.add_sh(rec, truth)
        for k, v in r.counters().items():
            self.c[k] = min(self.c[k], v) if k == "corner_worst" else self.c[k] + v

    def add_sh(self, rec, truth):
        v, _ = evaluate("sh", rec)
        sph = rec[:, 24] != 0
        d = ~sph
        self._add("sphere_relevant<true>", v[sph] & 1, truth[sph], rec[sph])
        self._add("sphere_relevant<false>", v[d] & 1, truth[d], rec[d])
        self._add("crec_relevant", (v[d] >> 1) & 1, truth[d], rec[d])
        self._add("crec_in_box_shadow", (v[d] >> 2) & 1, truth[d], rec[d])
        self.crec_differs += int(((v[d] & 1) != ((v[d] >> 1) & 1)).sum())
        self.box_overloads_differ += int((((v[d] >> 2) & 1) != ((v[d] >> 3) & 1)).sum())
        nf = ~np.isfinite(rec[:, 4])
        self.nonfinite_culled += int((v[nf & sph] != 1).sum() + (v[nf & d] != 15).sum())

    def table(self):
        lines = [f"{p:24s} cases {self.n[p]:9d}  culled {self.culled[p]:9d}  oracle accepts {self.accepts[p]:9d}  unsound {self.unsound[p]:3d}" for p in PREDICATES]
        c = self.c
        lines.append(f"corner claim: {c['corner_n']} lanes, {c['corner_bad']} below cos_t (1 - 1e-9), smallest dot / cos_t - 1 = {c['corner_worst'] - 1.0:.3e}")
        lines.append(f"own-sphere window: {c['own_n']} rays, {c['own_skip']} inside, {c['own_bad']} blocked;  backface skips: {c['bf_n']} terms, {c['bf_skip']} skipped, {c['bf_bad']} not inert, {c['bf_negzero']} of the rest -0")
        lines.append(f"equalities: crec_relevant != sphere_relevant<false> {self.crec_differs}, box overloads differ {self.box_overloads_differ}, "
                     f"non-finite radius culled {self.nonfinite_culled}")
        return "\n".join(lines)

    def total_unsound(self):
        return sum(self.unsound.values()) + self.c["corner_bad"] + self.c["own_bad"] + self.c["bf_bad"] + self.crec_differs + self.box_overloads_differ + self.nonfinite_culled


# ---- source 1: real frames ------------------------------------------------------------------------------------------------------
def sphere(c, r):
    out = (C.c_double * 20)()
    O.lib().orc_surface_sphere(O._d3(c), float(r), out)
    return list(out)


def plane(o, n):
    out = (C.c_double * 20)()
    O.lib().orc_surface_plane(O._d3(o), O._d3(n), out)
    return list(out)


def add_light(s, kind, v, color, intensity):
    l = O.OrcLight()
    (O.lib().orc_light_directional if kind == "directional" else O.lib().orc_light_spherical)(C.c_float(float(intensity)), O._d3(v), O._f3(color), C.byref(l))
    s.lights.append(l)


def fuzz_scene(seed):
    """tests/tools/fuzz_parity.py's scene(seed) -- the same draws in the same order -- on the oracle's scene class (no GPU library needed)."""
    rng = np.random.default_rng(77000 + seed)
    w, h = int(rng.integers(1, 140)), int(rng.integers(1, 100))
    s = O.Scene(w, h, float(rng.uniform(10, 110)), int(rng.integers(0, 5)), rng.uniform(0, 1, 3))
    n_obj = int(rng.integers(0, 30))
    scale = float(10 ** rng.uniform(-1, 2))
    for i in range(n_obj):
        kind = int(rng.integers(0, 6))
        refl = float(rng.uniform(0.05, 1.0)) if rng.random() < 0.25 else 0.0
        col = rng.uniform(0, 1, 3)
        if kind <= 2:
            c = rng.uniform([-12, -8, -5], [12, 8, 40]) * scale
            r = float(10 ** rng.uniform(-1.5, 1.0)) * scale
            s.add_object(sphere(c, r), col, refl)
        elif kind == 3:
            q = np.zeros(20)
            q[10:13] = rng.uniform(-2, 2, 3)
            if rng.random() < 0.5:
                q[13:16] = rng.uniform(-1, 1, 3)
            c = rng.uniform([-6, -4, 4], [6, 4, 25]) * scale
            q[16:19] = -2.0 * q[10:13] * c
            q[19] = float(np.dot(q[10:13], c * c) - rng.uniform(0.2, 8.0) * scale * scale)
            s.add_object(q, col, refl)
        elif kind == 4:
            n = rng.normal(size=3)
            s.add_object(plane(rng.uniform(-8, 8, 3) * scale, n), col, refl)
        else:
            q = np.zeros(20)
            q[10:13] = 1.0
            q[16:19] = rng.uniform(-4, 4, 3)
            q[19] = float(rng.uniform(0, 50))
            s.add_object(q, col, refl)
    for i in range(int(rng.integers(0, 9))):
        if rng.random() < 0.5:
            add_light(s, "directional", rng.normal(size=3), rng.uniform(0, 1, 3), float(rng.uniform(0, 2)))
        else:
            add_light(s, "spherical", rng.uniform([-15, -10, -10], [15, 20, 40]) * scale, rng.uniform(0, 1, 3), float(rng.uniform(1, 900)) * scale * scale)
    cam = O.camera_matrix(pos=rng.uniform(-3, 3, 3) * scale, yaw_deg=float(rng.uniform(60, 120)), pitch_deg=float(rng.uniform(-25, 25)))
    return s, cam


def sphere_field(seed, n_spheres, n_lights, w, h, shift=(0.0, 0.0, 0.0), with_plane=False):
    """The ranges of test_gpu_parity.random_scene."""
    rng = np.random.default_rng(seed)
    s = O.Scene(w, h, float(rng.uniform(30, 80)), 0, (0.1, 0.2, 0.3))
    shift = np.asarray(shift, dtype=np.float64)
    for i in range(n_spheres):
        c = rng.uniform([-12, -6, 6], [12, 8, 40])
        s.add_object(sphere(c + shift, float(rng.uniform(0.3, 3.0))), rng.uniform(0, 1, 3), 0.0)
    if with_plane:
        s.add_object(plane(np.array([0, -7.0, 0]) + shift, [0.05, 1, 0.02]), (0.5, 0.5, 0.5), 0.0)
    for i in range(n_lights):
        if i % 2 == 0:
            add_light(s, "directional", rng.normal(size=3) + np.array([0, -1.5, 0]), rng.uniform(0, 1, 3), float(rng.uniform(0.2, 1.5)))
        else:
            add_light(s, "spherical", rng.uniform([-15, 0, 0], [15, 20, 40]) + shift, rng.uniform(0, 1, 3), float(rng.uniform(100, 900)))
    return s


def general_camera(rng, pos, mirrored):
    """A scaled and sheared camera matrix (test_gpu_parity.general_camera_case), column-major."""
    base = O.camera_matrix(pos, float(rng.uniform(70, 110)), float(rng.uniform(-10, 10))).reshape(4, 4).T.copy()
    lin = np.eye(3) + rng.normal(scale=0.25, size=(3, 3))
    if mirrored:
        lin[:, 0] *= -1.0
    m = base.copy()
    m[:3, :3] = base[:3, :3] @ lin
    return np.ascontiguousarray(m.T).reshape(16)


def mixed_scene(seed, w=96, h=72):
    """The classes of test_gpu_parity.mixed_scene: spheres, general quadrics, planes, both light kinds."""
    rng = np.random.default_rng(1000 + seed)
    s = O.Scene(w, h, float(rng.uniform(35, 75)), 0, rng.uniform(0, 1, 3))
    for i in range(int(rng.integers(4, 14))):
        kind = rng.integers(0, 4)
        col = rng.uniform(0, 1, 3)
        if kind <= 1:
            s.add_object(sphere(rng.uniform([-10, -6, 5], [10, 8, 35]), float(rng.uniform(0.3, 3.0))), col, 0.0)
        elif kind == 2:
            q = np.zeros(20)
            q[10:13] = rng.uniform(-1.5, 2.0, 3)
            if rng.random() < 0.5:
                q[13:16] = rng.uniform(-0.5, 0.5, 3)
            c = rng.uniform([-6, -4, 8], [6, 4, 25])
            q[16:19] = -2.0 * q[10:13] * c
            q[19] = float(np.dot(q[10:13], c * c) - rng.uniform(0.5, 6.0))
            s.add_object(q, col, 0.0)
        else:
            n = rng.normal(size=3)
            s.add_object(plane(rng.uniform([-5, -8, 0], [5, -3, 30]), n / np.linalg.norm(n) + np.array([0, 1.5, 0])), col, 0.0)
    for i in range(int(rng.integers(1, 6))):
        if rng.random() < 0.5:
            add_light(s, "directional", rng.normal(size=3) + np.array([0, -1.2, 0]), rng.uniform(0, 1, 3), float(rng.uniform(0.3, 1.5)))
        else:
            add_light(s, "spherical", rng.uniform([-12, -2, -5], [12, 15, 35]), rng.uniform(0, 1, 3), float(rng.uniform(100, 900)))
    return s


def frame_sources(n_fuzz=12, small=True):
    """(name, scene, camera, stride): the shipped degree <= 2 scenes, fuzz_parity scenes (seeds 158 and 534 among them), mixed-class scenes,
    sphere fields under general cameras, the 1e6-translated field, raw-descriptor scenes with odd light vectors and non-finite colours."""
    import raw_desc_scenes as RD
    w, h = (96, 72) if small else (256, 192)
    for name in ("quadratic", "20spheres", "reflection_test"):
        yield name, O.load_scene(os.path.join(ROOT, "scenes", name + ".yml")).with_size(w, h), None, 3
    for seed in [158, 534] + list(range(n_fuzz)):
        s, cam = fuzz_scene(seed)
        yield f"fuzz {seed}", s, cam, 3
    for seed in range(4):
        yield f"mixed {seed}", mixed_scene(seed), None, 3
    for seed in range(6):
        rng = np.random.default_rng(9100 + seed)
        s = sphere_field(9100 + seed, int(rng.integers(4, 30)), int(rng.integers(1, 7)), 104 + 8 * seed + seed, 70 + seed)
        yield f"general camera {seed}", s, general_camera(rng, (float(rng.uniform(-3, 3)), float(rng.uniform(-2, 2)), float(rng.uniform(-4, 2))), seed % 3 == 0), 3
    for seed in range(4):     # many blocks and tiles: the per-block and per-tile predicates get their share of verdicts here
        rng = np.random.default_rng(4200 + seed)
        yield f"large field {seed}", sphere_field(4200 + seed, 40, 3, 512, 384), (None if seed == 0 else general_camera(rng, (0.5 * seed, 0.2, -1.0), seed == 3)), 16
    shift = (1e6, -2e6, 5e5)
    yield "translated 1e6", sphere_field(77, 16, 4, w, h, shift=shift), O.camera_matrix(pos=shift), 3
    for seed in range(0, RD.N_SEEDS, 3):
        s, cam = RD.scene(seed)
        if not any(any(c != 0 for c in o.c[:10]) for o in s.objects):
            t = s.with_size(min(s.width, 96), min(s.height, 72))
            yield f"raw descriptor {seed}", t, cam, 3


# ---- source 2: the grazing generator ---------------------------------------------------------------------------------------------
def _clearance(rng, n):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** (-rng.integers(1, 16, n).astype(np.float64))


def graze_primary_params(n, seed, mode):
    """Parameters of lab_graze_primary: scene scales 1e-2 .. 1e6, camera translations up to 1e7, radii 1e-4 .. 10 scales, pixel pitches 1e-3.5
    .. 1e-0.5 (a sixth wider still: cones with cos_t down to 0.2 and below), rigid / scaled / sheared / mirrored cameras."""
    rng = np.random.default_rng(510000 + seed)
    par = np.zeros((n, GP_W))
    for i in range(n):
        H = int(rng.integers(8, 120))
        W = int(rng.integers(8, 160))
        pitch = 10.0 ** rng.uniform(-3.5, -0.5) if rng.random() < 5 / 6 else rng.uniform(0.3, 0.9)
        fov = 2.0 * np.arctan(0.5 * pitch * H)
        scale = 10.0 ** rng.uniform(-2, 6)
        pos = rng.normal(size=3) * (0.0 if rng.random() < 0.2 else 10.0 ** rng.uniform(0, 7))
        kind = int(rng.integers(0, 4))
        cam = O.camera_matrix(pos, float(rng.uniform(0, 360)), float(rng.uniform(-60, 60))) if kind == 0 else general_camera(rng, pos, kind == 3)
        bx, by = int(rng.integers(0, (W + 7) // 8)), int(rng.integers(0, (H + 7) // 8))
        if mode == 0:
            lane = int(rng.choice([0, 7, 56, 63])) if rng.random() < 0.5 else int(rng.choice([int(rng.integers(0, 8)), 56 + int(rng.integers(0, 8)), 8 * int(rng.integers(0, 8)), 8 * int(rng.integers(0, 8)) + 7]))
        else:
            lane = int(rng.integers(0, 64))
        s = min(scale * 10.0 ** rng.uniform(-1, 1), 4e5)
        r = scale * 10.0 ** rng.uniform(-4, 1)
        if rng.random() < 0.9:
            r = min(r, s * 10.0 ** rng.uniform(-3, -0.3))      # (else the ray origin often lies inside the sphere: every ray accepts)
        par[i, :3] = (W, H, fov)
        par[i, 3:19] = cam
        par[i, 19:26] = (bx, by, lane, s, r, 0.0, mode)
    par[:, 24] = _clearance(rng, n)
    return par


def graze_primary(n, seed, mode):
    lib = build()
    par = graze_primary_params(n, seed, mode)
    r = Records({"cone": n, "pyr": n})
    centre = np.zeros((n, 3))
    lib.lab_graze_primary(n, _dp(par), C.byref(r.out), _dp(centre))
    return r, par, centre


def graze_shadow_params(n, seed, spherical):
    """Parameters of lab_graze_shadow.  The chunk: up to 64 hits in a box (some thin and long: a near and a far sphere), its corners among
    them, so that a sphere tangent to a corner's ray is tangent to the box's shadow hexagon and to the ball-swept line.  Directional lights:
    any direction, a third of them nearly parallel to a box axis.  Point lights: far, near, inside or next to the chunk's ball; the tangent
    point near the ray's origin (we = 0), near the light (we = ee) or between."""
    rng = np.random.default_rng(520000 + seed + (7 if spherical else 0))
    par = np.zeros((n, GS_W))
    for i in range(n):
        scale = 10.0 ** rng.uniform(-2, 6)
        centre = rng.normal(size=3) * (0.0 if rng.random() < 0.2 else 10.0 ** rng.uniform(0, 7))
        half = scale * 10.0 ** rng.uniform(-3, 0, 3)
        if rng.random() < 0.4:
            half[int(rng.integers(0, 3))] = scale * 10.0 ** rng.uniform(0, 1.5)    # long and thin
        m = int(rng.integers(1, 65))
        pts = centre + half * rng.uniform(-1, 1, (m, 3))
        corners = centre + half * rng.choice([-1.0, 1.0], (min(m, 8), 3))
        pts[:len(corners)] = corners
        nrm = rng.normal(size=(m, 3))
        j = int(rng.integers(0, min(m, 8))) if rng.random() < 0.7 else int(rng.integers(0, m))
        r = scale * 10.0 ** rng.uniform(-4, 1)
        if spherical:
            u = rng.random()
            reach = np.linalg.norm(half) + 1e-2
            if u < 0.3:
                lp = centre + rng.normal(size=3) / np.sqrt(3) * reach * rng.uniform(0, 1.5)      # inside or next to the ball
            else:
                lp = centre + rng.normal(size=3) * scale * 10.0 ** rng.uniform(-1, 2)
            v = rng.random()
            k = 10.0 ** (-rng.integers(1, 9))
            s = rng.uniform(0, 1) if v < 0.4 else (rng.choice([-1.0, 1.0]) * k if v < 0.7 else 1.0 + rng.choice([-1.0, 1.0]) * k)
            dlen = np.linalg.norm(lp - pts[j])
            if rng.random() < 0.5 and dlen > 0:      # the sphere's cap at the end of the segment: tangent point a radius before / behind the end
                s = s + (r / dlen) * rng.choice([-1.0, 1.0])
        else:
            lp = rng.normal(size=3)
            if rng.random() < 1 / 3:
                lp = np.zeros(3)
                lp[int(rng.integers(0, 3))] = rng.choice([-1.0, 1.0])
                lp += rng.normal(size=3) * 10.0 ** (-rng.integers(1, 12))
            lp = lp / np.linalg.norm(lp) * (1.0 if rng.random() < 0.7 else 10.0 ** rng.uniform(-2, 2))
            dist = scale * 10.0 ** rng.uniform(-2, 2) * (1.0 if rng.random() < 0.85 else -1.0)
            s = dist / np.linalg.norm(lp)
        par[i, 0] = 1.0 if spherical else 0.0
        par[i, 1:4] = lp
        par[i, 4:10] = (r, 0.0, s, rng.uniform(0, 2 * np.pi), j, m)
        par[i, 10:10 + 6 * m] = np.concatenate([pts, nrm], axis=1).reshape(-1)
    par[:, 5] = _clearance(rng, n)
    return par


def graze_shadow(n, seed, spherical):
    lib = build()
    par = graze_shadow_params(n, seed, spherical)
    r = Records({"sh": n})
    centre = np.zeros((n, 3))
    lib.lab_graze_shadow(n, _dp(par), C.byref(r.out), _dp(centre))
    return r, par, centre


def hand_made_solve_records():
    """us_needs_solve / needs_solve on hand-made coefficients.  The truth is orc_intersect_ray on the surface t2 x^2 + t1 x + t0 = 0 along the
    ray o = 0, d = (1, 0, 0), whose polynomial has exactly these coefficients."""
    tiny = [5e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 1e-200, 1e-100, 1e-30, 1e-16, 9.9e-8, 1e-7, np.nextafter(1e-7, 1), 1.1e-7, 1e-3, 1.0, 1e10, 1e150, 1e300]
    cases = []
    for t2 in [np.nextafter(1e-7, 0), 1e-7, np.nextafter(1e-7, 1), 1e-3, 1.0, 4.0, 1e10, 1e150]:
        for t1 in tiny + [-x for x in tiny] + [0.0]:
            for t0 in tiny + [-x for x in tiny] + [0.0]:
                cases.append((t2, t1, t0))
        for t1 in (1.0, -1.0, 3.0, -1e5, 1e-5):   # discriminants one ulp either side of 0
            t0 = t1 * t1 / (4.0 * t2)
            for k in (t0, np.nextafter(t0, np.inf), np.nextafter(t0, -np.inf), np.nextafter(np.nextafter(t0, np.inf), np.inf)):
                cases.append((t2, t1, float(k)))
    lib = build()
    us, gq = [], []
    o, d = np.zeros(3), np.array([1.0, 0.0, 0.0])
    with np.errstate(over="ignore", invalid="ignore"):
        for t2, t1, t0 in cases:
            coef = np.zeros(20)
            coef[10], coef[16], coef[19] = t2, t1, t0
            t = lib.lab_oracle_root(_dp(coef), _dp(o), _dp(d))
            us.append((1.0 if abs(t2) > EPS else 0.0, 4.0 * t2, t1, t0, t))
            gq.append((t2, t1, t0, t))
    return np.array(us), np.array(gq)


# ---- whole scenes for the product kernels: a sphere set tangent to a block's cone, a tile's pyramid or a chunk's shadow volume -------------
GRAZE_KINDS = ("cone", "pyramid", "shadow_directional", "shadow_point")
N_GRAZE_SCENES = 32


def graze_scene_spec(i, with_tangent=True):
    """Scene i as plain data: {"w", "h", "fov", "spheres": [(centre, radius, colour)], "lights": [(kind, vector, colour, intensity)], "kind"}.
    All spheres (>= 4 of them cullable, no mirrors: both instantiations render it), the camera at the origin looking along +z.  Five base
    spheres -- a near one in front of a far, large one, so that blocks on the near one's silhouette form chunks spanning both -- and six
    spheres tangent, at clearances +-1e-1 ... +-1e-15, to a corner / edge ray of an 8 x 8 block, an edge ray of a 16 x 16 tile, or the shadow
    ray of a hit on the near sphere or the far one towards a directional or the point light."""
    kind = GRAZE_KINDS[i % 4]
    rng = np.random.default_rng(640000 + i)
    w, h, fov = 128, 96, 50.0
    base = [((-1.5, 0.0, 8.0), 1.2), ((-1.0, 0.3, 24.0), 5.0), ((3.0, 1.0, 12.0), 1.0), ((2.0, -2.0, 9.0), 0.7), ((-4.0, 2.0, 15.0), 1.5)]
    spheres = [(tuple(np.array(c) + rng.normal(scale=0.2, size=3)), r * float(rng.uniform(0.9, 1.1)), tuple(rng.uniform(0.2, 1, 3))) for c, r in base]
    lights = [("directional", tuple(np.array([0.3, -1.0, 0.2]) + rng.normal(scale=0.15, size=3)), (1.0, 0.9, 0.8), 0.8),
              ("directional", tuple(np.array([-0.6, -0.5, 0.6]) + rng.normal(scale=0.15, size=3)), (0.6, 0.7, 1.0), 0.6),
              ("spherical", tuple(np.array([2.0, 9.0, 4.0]) + rng.normal(scale=0.5, size=3)), (1.0, 1.0, 1.0), 300.0)]
    spec = {"w": w, "h": h, "fov": fov, "spheres": spheres, "lights": lights, "kind": kind, "n_base": len(spheres)}
    if not with_tangent:
        return spec
    deltas = rng.choice([-1.0, 1.0], 6) * 10.0 ** (-((np.arange(6) * 5 + i // 4 * 2 + rng.integers(0, 2, 6)) % 15 + 1).astype(np.float64))
    osc = spec_to_oracle(spec)
    centres = []
    if kind in ("cone", "pyramid"):
        par = np.zeros((6, GP_W))
        par[:, :3] = (w, h, osc.vertical_fov)
        par[:, 3:19] = O.IDENTITY
        for k in range(6):
            lane = int(rng.choice([0, 7, 56, 63])) if kind == "cone" and k % 2 == 0 else int(rng.integers(0, 64))
            r = 10.0 ** rng.uniform(-1.3, -0.2)
            par[k, 19:26] = (int(rng.integers(1, w // 8 - 1)), int(rng.integers(1, h // 8 - 1)), lane, float(rng.uniform(4, 20)), r, deltas[k], 0 if kind == "cone" else 1)
        out = Records({"cone": 6, "pyr": 6})
        c = np.zeros((6, 3))
        build().lab_graze_primary(6, _dp(par), C.byref(out.out), _dp(c))
        centres = [(tuple(c[k]), float(par[k, 23])) for k in range(6)]
    else:
        lib, sc = O.lib(), osc.c_scene()
        cam = np.ascontiguousarray(O.IDENTITY)
        li = int(rng.integers(0, 2)) if kind == "shadow_directional" else 2
        light = osc.lights[li]
        hits = []     # (surface point, biased origin) of pixels on the near sphere and the far one that face the light
        for y in range(2, h, 3):
            for x in range(2, w, 3):
                d = (C.c_double * 3)()
                lib.orc_primary_dir(C.byref(sc), _dp(cam), x, y, d)
                best, bt = -1, np.inf
                for k in range(2):
                    t = lib.orc_intersect_ray(osc.objects[k].c, O._d3((0, 0, 0)), d)
                    if EPS <= t < MAX_T and t < bt:
                        best, bt = k, t
                if best < 0:
                    continue
                pt = np.array([bt * d[0], bt * d[1], bt * d[2]])
                n = (C.c_double * 3)()
                lib.orc_normal_vector(osc.objects[best].c, O._d3(pt), n)
                n = np.array(list(n))
                fd, mt = (C.c_float * 3)(), C.c_double()
                lib.orc_shadow_ray(C.byref(light), O._d3(pt), fd, C.byref(mt))
                dv = np.array([fd[0], fd[1], fd[2]], dtype=np.float64)
                if float(n @ dv) > 0.05 * np.linalg.norm(dv):
                    hits.append((pt + 1e-2 * n, dv))
        assert len(hits) >= 6, (i, len(hits))
        for k in range(6):
            so, dv = hits[int(rng.integers(0, len(hits)))]
            r = 10.0 ** rng.uniform(-1.3, -0.2)
            s = float(rng.uniform(1.5, 6.0)) / np.linalg.norm(dv) if kind == "shadow_directional" else float(rng.uniform(0.1, 0.9))
            a = np.cross(dv, rng.normal(size=3))
            a /= np.linalg.norm(a)
            centres.append((tuple(so + s * dv + r * (1.0 + deltas[k]) * a), float(r)))
    spec["spheres"] = spheres + [(c, r, tuple(rng.uniform(0.2, 1, 3))) for c, r in centres]
    return spec


def spec_to_oracle(spec):
    s = O.Scene(spec["w"], spec["h"], spec["fov"], 0, (0.1, 0.2, 0.3))
    for c, r, col in spec["spheres"]:
        s.add_object(sphere(c, r), col, 0.0)
    for kind, v, col, intensity in spec["lights"]:
        add_light(s, kind, v, col, intensity)
    return s


def tangent_spheres_decide(spec):
    """With the oracle alone: does the frame change when the tangent spheres are taken out, i.e. is one of them the nearest hit or the sole
    blocker of some pixel?"""
    full = spec_to_oracle(spec).render(nthreads=4)
    bare = dict(spec, spheres=spec["spheres"][:spec["n_base"]])
    return not np.array_equal(full, spec_to_oracle(bare).render(nthreads=4))


def graze_scenes():
    """The scenes whose tangent spheres decide a pixel (the others are dropped), and how many were generated."""
    specs = [graze_scene_spec(i) for i in range(N_GRAZE_SCENES)]
    return [s for s in specs if tangent_spheres_decide(s)], len(specs)


def margin_pins():
    """Hand-made shadow records that pin the documented margins, with the verdict bits (lab_eval_sh) they must give.
    * ball stage: a unit sphere whose centre lies r + R + 1e-7 (w1 + r + R + 1) from the chunk's axis -- inside the 1e-6 margin of
      cull_record / sphere_relevant, a hundred times outside a 1e-9 one: kept by both.  At r + R + 1e-5 (...): culled by both.
    * box stage: the light along +z, so the first hexagon normal reads |w.y| <= (h.y + limr) (1 + 1e-9).  With w.y half a part in 1e9
      above h.y + limr the sphere is kept only because of that factor; two parts in 1e9 above, it is culled."""
    def rec(wy, hy, R):
        c = np.array([0.0, wy, 0.0])
        r = np.zeros(REC["sh"])
        r[0:3] = -2.0 * c
        r[3] = float(c @ c) - 1.0
        r[4], r[5] = 1.0, 1.0
        r[9] = R
        r[10:13] = (0.5, hy, 0.5)
        r[13:16] = r[16:19] = (0.0, 0.0, 1.0)
        r[19], r[20] = 1.0, 1.001
        r[21:24] = (1.0, 1.0, 0.0)
        return r
    pins = []
    R = 3.0
    for k, keep in ((1e-7, True), (1e-5, False)):
        wy = (1.0 + R) / (1.0 - k) + k * (2.0 + R) / (1.0 - k)      # wy = 1 + R + k (wy + 1 + R + 1)
        pins.append((rec(wy, 20.0, R), 3, 3 if keep else 0, f"ball stage, {k:g} of the distances outside r + R"))
    wy, R = 10.0, 20.0
    _, crec = evaluate("sh", rec(wy, 1.0, R))
    limr = float(crec[0, 5])
    for k, keep in ((5e-10, True), (2e-9, False)):
        pins.append((rec(wy, wy / (1.0 + k) - limr, R), 12, 12 if keep else 0, f"box stage, {k:g} above the hexagon's bound"))
    return pins


# ---- non-vacuity: exact distance from the predicate's own bounding volume (mpmath, 50 digits) -------------------------------------
def exact_excess(kind, rec):
    """(distance of the centre from the predicate's bounding volume) - r, and the predicate's distance scale (the bracket its 1e-6 multiplies
    plus (s2 + 1) * 1e-6 / r), for one record.  None where the predicate never culls (cone wider than cos_t = 0.2, non-finite radius)."""
    import mpmath as mp
    mp.mp.dps = 50
    f = [mp.mpf(float(x)) for x in rec]
    V = lambda a: mp.matrix(a)
    dot = lambda a, b: sum(x * y for x, y in zip(a, b))
    if kind in ("cone", "pyr"):
        k, r, org = f[0:3], f[3], f[5:8]
        if not np.isfinite(rec[3]):
            return None
        c = [-x / 2 for x in k]
        v = [a - b for a, b in zip(c, org)]
        v1 = sum(abs(x) for x in v)
        s2 = dot(c, c) + dot(org, org)
        scale = v1 + r + 1 + (s2 + 1) * mp.mpf(1e-6) / r
        if kind == "cone":
            if not rec[11] > 0.2:
                return None
            a = f[8:11]
            an = mp.sqrt(dot(a, a))
            h = dot(v, a) / an
            rho = mp.sqrt(max(dot(v, v) - h * h, 0))
            ct = f[11] * (1 - mp.mpf(1e-9)) / an       # the widened cone of the predicate (axis renormalised: the kernel's is a unit vector up to rounding)
            st = mp.sqrt(1 - ct * ct)
            # The predicate's own volume is bounded by the cone's generator LINES (rt_wavefront_math.hpp: "signed distance of the centre
            # from the cone's generator line, never larger than its distance to the cone"), not by the cone: behind the apex the lines run
            # on, and a sphere there is kept although it is far from every ray (measured: kept at 0.108 of the distance scale beyond the true
            # cone, a sphere of radius 41 behind the camera of fuzz scene 1).  The distance asked of it is therefore the one to the lines.
            dist = max(rho * ct - h * st, mp.mpf(0))
            return float(dist - r), float(scale)
        nt, (cx0, cx1, cy0, cy1) = f[8:17], f[17:21]
        c0, c1, c2 = nt[0:3], nt[3:6], nt[6:9]
        planes = [[a - cx0 * b for a, b in zip(c0, c2)], [cx1 * b - a for a, b in zip(c0, c2)], [a - cy0 * b for a, b in zip(c1, c2)],
                  [cy1 * b - a for a, b in zip(c1, c2)], c2]
        dist = max(-dot(n, v) / mp.sqrt(dot(n, n)) for n in planes)
        return float(dist - r), float(scale)
    k, r, bc, R = f[0:3], f[4], f[6:9], f[9]
    if not np.isfinite(rec[4]):
        return None
    c = [-x / 2 for x in k]
    w = [a - b for a, b in zip(c, bc)]
    w1 = sum(abs(x) for x in w)
    s2 = dot(c, c) + dot(bc, bc)
    if kind == "sh_dir":       # the ball swept along the line through its centre
        u = f[16:19]
        along = dot(w, u) / mp.sqrt(dot(u, u))
        perp = mp.sqrt(max(dot(w, w) - along * along, 0))
        scale = w1 + r + R + 1 + (s2 + 1) * mp.mpf(1e-6) / r
        return float(perp - R - r), float(scale)
    if kind == "sh_box":       # crec_in_box_shadow's own volume: the box's shadow along sdir, measured along each hexagon normal sdir x e_k in
        u, hh = f[16:19], f[10:13]      # the 1-norm the predicate bounds |sdir x e_k| with (so up to sqrt 2 more generous than the Euclidean prism)
        normals = ([0, u[2], -u[1]], [-u[2], 0, u[0]], [u[1], -u[0], 0])
        worst = None
        for n in normals:
            n1 = sum(abs(x) for x in n)
            if n1 == 0:
                continue
            e = (abs(dot(w, n)) - sum(h * abs(x) for h, x in zip(hh, n))) / n1
            worst = e if worst is None or e > worst else worst
        scale = w1 + r + R + 1 + (s2 + 1) * mp.mpf(1e-6) / r
        return (None if worst is None else (float(worst - r), float(scale)))
    if kind == "sh_sph":       # the ball swept along the segment to the light
        p = f[13:16]
        e = [a - b for a, b in zip(p, bc)]
        ee = dot(e, e)
        tpar = 0 if ee == 0 else min(max(dot(w, e) / ee, 0), 1)
        q = [a - tpar * b for a, b in zip(w, e)]
        e1 = sum(abs(x) for x in e)
        scale = w1 + r + R + e1 + 1 + (s2 + dot(p, p) + 1) * mp.mpf(1e-6) / r
        return float(mp.sqrt(dot(q, q)) - R - r), float(scale)
    raise ValueError(kind)


def must_cull_failures(kind, rec, verdict, sample=1500, seed=0, band=1e-3):
    """Of a sample of records: how many lie beyond the band (exact excess > band * scale) and are still answered "test it"; also returns how
    many of the sample lay beyond the band at all."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(len(rec), min(sample, len(rec)), replace=False)
    beyond = kept = 0
    for i in idx:
        x = exact_excess(kind, rec[i])
        if x is None:
            continue
        excess, scale = x
        if excess > band * scale:
            beyond += 1
            kept += int(verdict[i] != 0)
    return kept, beyond


def smallest_culled_clearance(verdict, par_delta):
    c = np.abs(par_delta[(verdict == 0)])
    return float(c.min()) if len(c) else float("nan")


def run(n, first_seed=0, chunk=20000, verbose=True):
    """n grazing cases per family (cone, pyramid, directional, point), in chunks; returns (Tally, smallest culled clearance per family)."""
    t = Tally()
    small = {}
    for name, fn in (("cone", lambda k, s: graze_primary(k, s, 0)), ("pyramid", lambda k, s: graze_primary(k, s, 1)),
                     ("directional", lambda k, s: graze_shadow(k, s, False)), ("point", lambda k, s: graze_shadow(k, s, True))):
        done, s = 0, first_seed
        small[name] = float("inf")
        while done < n:
            k = min(chunk, n - done)
            r, par, _ = fn(k, s)
            t.add(r)
            kind = {"cone": "cone", "pyramid": "pyr"}.get(name, "sh")
            rec, _ = r.get(kind)
            v = evaluate(kind, rec)
            v = v[0] if kind == "sh" else v
            delta = par[:, 24] if kind != "sh" else par[:, 5]
            if len(rec) == len(par):
                cull = (v & (1 if kind != "sh" or name == "point" else 7)) != (1 if kind != "sh" or name == "point" else 7)
                pos = cull & (delta > 0)
                if pos.any():
                    small[name] = min(small[name], float(delta[pos].min()))
            done += k
            s += 1
    return t, small


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    t0 = time.time()
    frames = Tally()
    for name, s, cam, stride in frame_sources(n_fuzz=40):
        frames.add(frame(s, cam, stride=stride))
    print("real frames:")
    print(frames.table())
    t, small = run(n, first)
    print(f"grazing generator, {n} cases per family from seed {first}:")
    print(t.table())
    print("smallest positive clearance culled: " + ", ".join(f"{k} {v:.0e}" for k, v in small.items()))
    print(f"cull_lab: {n} grazing cases per family, {sum(frames.n.values()) + sum(t.n.values())} verdicts, {frames.total_unsound() + t.total_unsound()} unsound, {time.time() - t0:.0f} s")
    sys.exit(1 if frames.total_unsound() + t.total_unsound() else 0)


if __name__ == "__main__":
    main()
