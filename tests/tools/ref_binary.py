"""Front end of the reference programs under oracle/_ref/ (test infrastructure).

oracle/Makefile.ref compiles the reference's own CPU path -- update-cpu.cpp, surface.cpp, light.cpp, scene-exception.cpp and the
header-only surface_impl.h / light_impl.h, unmodified -- with the drivers oracle/ref_driver.cpp (whole frames through init_update /
update) and oracle/ref_units.cpp (one reference function call per input row); the job formats are stated at the top of those two
files.  This module writes the jobs, runs one child process per call (a CPU program: it opens no GPU) and reads the results.

tests/test_oracle_vs_reference.py holds oracle/rt_oracle.c to these programs, tests/test_reference_gpu.py the kernels."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

POLYNOMIAL, SPHERE, PLANE, DINGDONG, CLEBSCH, CAYLEY = range(6)        # object kinds of oracle/ref_driver.cpp
STORED, DIRECTIONAL, SPHERICAL = range(3)                              # light kinds
OPS = {"intersect_ray": (1, 26, 1), "normal_vector": (2, 23, 3), "shadow_ray": (3, 7, 4), "surface_color": (4, 16, 3), "reflect_ray": (5, 6, 3),
       "sphere": (6, 4, 20), "plane": (7, 6, 20), "dingDong": (8, 3, 20), "clebsch": (9, 1, 20), "cayley": (10, 1, 20),
       "directional": (11, 7, 7), "spherical": (12, 7, 7)}           # name -> (op, input row, output row) of oracle/ref_units.cpp


class RefError(Exception):
    """A reference factory threw its SceneException (exit code 3); the text is the exception's."""


def available():
    """oracle/_ref/ with its four programs, built first where the reference tree is here.  Returns (directory or None, reason)."""
    d = O.build_ref()
    if d is not None:
        return d, ""
    if O.reference_present():
        return None, f"the reference tree is at {O.REFERENCE_DIR} but oracle/Makefile.ref left no programs in oracle/_ref/"
    return None, f"oracle/_ref/ holds no reference programs and the reference tree ({O.REFERENCE_DIR}) is absent too: nothing to build them from"


def require():
    """For a test: the directory of the programs.  Programs missing although the reference tree is here is a failure; both missing
    is the one case that skips."""
    import pytest
    d, why = available()
    if d is None:
        if O.reference_present():
            pytest.fail(why)
        pytest.skip(why)
    return d


def _run(program, job):
    with tempfile.TemporaryDirectory(prefix="rtref_") as tmp:
        jp, op = os.path.join(tmp, "job"), os.path.join(tmp, "out")
        with open(jp, "wb") as fh:
            fh.write(job)
        p = subprocess.run([os.path.join(O.REF_DIR, program), jp, op], capture_output=True, text=True)
        if p.returncode == 3:
            raise RefError(p.stderr.strip())
        if p.returncode != 0:
            raise RuntimeError(f"{program} exited with {p.returncode}: {p.stderr.strip()}")
        with open(op, "rb") as fh:
            return fh.read()


class RefScene:
    """A scene as oracle/ref_driver.cpp reads it: header fields as the reference's Scene holds them (vertical_fov in radians) and
    one record per object / light, either as stored or as arguments of the reference's factories."""

    def __init__(self, width, height, vertical_fov, max_reflections, bg_color):
        self.width, self.height, self.vertical_fov = int(width), int(height), float(vertical_fov)
        self.max_reflections = int(max_reflections)
        self.bg_color = np.asarray(bg_color, dtype=np.float32)
        self.objects, self.lights = [], []

    def add_object(self, kind, args, reflection_ratio, color):
        a = np.zeros(20, dtype=np.float64)
        a[:len(args)] = args
        self.objects.append((int(kind), a, np.float32(reflection_ratio), np.asarray(color, dtype=np.float32)))

    def add_light(self, kind, intensity, v, color):
        self.lights.append((int(kind), np.float32(intensity), np.asarray(v, dtype=np.float64), np.asarray(color, dtype=np.float32)))

    @classmethod
    def from_oracle(cls, sc):
        """Every object and light of an oracle Scene as stored: coefficients and light records bit for bit."""
        r = cls(sc.width, sc.height, sc.vertical_fov, sc.max_reflections, sc.bg_color)
        for o in sc.objects:
            r.add_object(POLYNOMIAL, list(o.c), o.reflection_ratio, list(o.color))
        for l in sc.lights:
            r.add_light(STORED, 1.0 if l.is_spherical else 0.0, list(l.p), list(l.color))
        return r

    @classmethod
    def from_yaml(cls, path):
        """A scene file of scenes/ with every surface and light built by the REFERENCE's factories from the file's arguments
        (surface.cpp, light.cpp); the header, the defaults and the syntax are the oracle loader's (the reference's YAML loader needs
        yaml-cpp and is not built)."""
        import yaml
        sc = O.load_scene(path)
        r = cls(sc.width, sc.height, sc.vertical_fov, sc.max_reflections, sc.bg_color)
        with open(path) as fh:
            d = yaml.safe_load(fh)
        zero = [0.0, 0.0, 0.0]
        for node in d["objects"]:
            t = node["type"]
            if t == "sphere":
                kind, args = SPHERE, O._vec3(node, "center", zero) + [float(node.get("radius", 1.0))]
            elif t == "plane":
                kind, args = PLANE, O._vec3(node, "origin", zero) + O._vec3(node, "normal", [0.0, 1.0, 0.0])
            elif t == "dingDong":
                kind, args = DINGDONG, O._vec3(node, "origin", zero)
            elif t in ("clebsch", "cayley"):
                kind, args = (CLEBSCH if t == "clebsch" else CAYLEY), []
            else:
                kind, args = POLYNOMIAL, [float(node["coefficients"].get(n, 0.0)) for n in O.COEF_NAMES]
            r.add_object(kind, args, node.get("reflection_ratio", 0.0), O._vec3(node, "color", required=True))
        for node in d["light_sources"]:
            kind, key = (DIRECTIONAL, "direction") if node["type"] == "directional" else (SPHERICAL, "position")
            r.add_light(kind, node.get("intensity", 1.0), O._vec3(node, key, required=True), O._vec3(node, "color", [1.0, 1.0, 1.0]))
        return r

    def job(self, cams, width=None, height=None, max_reflections=None):
        w, h = int(self.width if width is None else width), int(self.height if height is None else height)
        mr = int(self.max_reflections if max_reflections is None else max_reflections)
        out = [b"RTREFFRM", struct.pack("<6I", w, h, mr, len(self.objects), len(self.lights), len(cams)),
               struct.pack("<d3f", self.vertical_fov, *[float(x) for x in self.bg_color])]
        for kind, a, refl, col in self.objects:
            out += [struct.pack("<I", kind), a.astype("<f8").tobytes(), struct.pack("<4f", float(refl), *[float(x) for x in col])]
        for kind, intensity, v, col in self.lights:
            out += [struct.pack("<If", kind, float(intensity)), v.astype("<f8").tobytes(), struct.pack("<3f", *[float(x) for x in col])]
        for cam in cams:
            out.append(np.ascontiguousarray(O.IDENTITY if cam is None else cam, dtype="<f8").reshape(16).tobytes())
        return b"".join(out), (len(cams), h, w, 3)

    def render(self, cams, width=None, height=None, max_reflections=None, opt="O2"):
        """float32 [len(cams), H, W, 3] from the reference's update(), row 0 = bottom; a camera of None is the identity."""
        job, shape = self.job(cams, width, height, max_reflections)
        return np.frombuffer(_run("ref_frames_" + opt, job), dtype="<f4").reshape(shape).copy()


def render(sc, cams, opt="O2", **size):
    """The reference's frames of an oracle Scene (objects and lights as stored)."""
    return RefScene.from_oracle(sc).render(cams, opt=opt, **size)


def units(name, rows, opt="O2"):
    """One call of the reference function `name` (a key of OPS) per row: float64 [n, k] -> float64 [n, m]."""
    op, k, m = OPS[name]
    rows = np.ascontiguousarray(rows, dtype="<f8").reshape(-1, k)
    out = _run("ref_units_" + opt, b"RTREFUNI" + struct.pack("<IIQ", op, k, len(rows)) + rows.tobytes())
    return np.frombuffer(out, dtype="<f8").reshape(len(rows), m).copy()


def same_bits(a, b):
    """array_equal on the raw bits, except that a NaN only has to be a NaN on both sides (sign and payload of a NaN are not values)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(u), b[~nb].view(u)))
