#!/usr/bin/env python3
"""The degree-3 path of rt_math.hpp on gfx950, ray by ray, against the oracle (test infrastructure; tests/test_cubic_device.py).

tests/tools/cubic_device_lab.hip runs the kernels' own header in plain kernels: the device's cbrt / acos / cos on a batch of
arguments (lab_libm), intersect_cubic_taylor / intersect_cubic_branch / cubic_guarded on ray records (lab_rays) and cubic_guarded
on hand-made polynomials (lab_guard).  The ray records are every degree-3 test of a frame as the oracle makes it
(tests/tools/cubic_guard_lab.cpp, lab_enumerate).  render_device_libm renders the oracle with the device's cbrt / acos / cos in its
solver, so that the dense path can be held to bit-identity and whole frames to zero pixels beyond 1e-5.

usage: python tests/tools/cubic_device_lab.py [scene ...]     (needs a GPU)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import cubic_guard_lab as CPU  # noqa: E402  (the CPU lab: the oracle, the enumeration of the tests, fuzz_scene)

O = CPU.O
PKG_DIR = os.path.join(ROOT, "cuda-ray-tracer_amd")
SRC = os.path.join(HERE, "cubic_device_lab.hip")
SO = os.path.join(HERE, "bin", "libcubic_device_lab.so")
DEPS = [SRC, os.path.join(HERE, "cubic_lab_rays.h"), os.path.join(PKG_DIR, "Makefile"), os.path.join(PKG_DIR, "csrc", "rt_math.hpp"),
        os.path.join(PKG_DIR, "csrc", "rt_scene_dev.h"), os.path.join(ROOT, "include", "mi355rt.h")]

EPS = 1e-7
CUB_TOL = 1e-8   # rt_math.hpp: the relative uncertainty cubic_guarded allows an accepted root

# tests/tools/cubic_lab_rays.h and cubic_device_lab.hip (LabOut), restated
RAY = np.dtype([("o", "<f8", 3), ("d", "<f8", 3), ("max_t", "<f8"), ("rec", "<f8", 10), ("obj", "<i4"), ("flags", "<i4")])
WHERE = np.dtype([("kind", "<i4"), ("x", "<i4"), ("y", "<i4"), ("light", "<i4")])
OUT = np.dtype([("t", "<f8"), ("t_dense", "<f8"), ("t_guard", "<f8"), ("tc", "<f8", 4), ("refused", "<i4"), ("branch", "<i4"),
                ("guard_ok", "<i4"), ("pad", "<i4")])
assert RAY.itemsize == 144 and WHERE.itemsize == 16 and OUT.itemsize == 72
LAB_DECIDE, LAB_HAS_REC = 1, 2
KINDS = ("primary", "shadow", "bounce")
FN = {"cbrt": 0, "acos": 1, "cos": 2}


def devflags():
    """DEVFLAGS of cuda-ray-tracer_amd/Makefile, as make expands them (the strict variant adds -ffp-contract=off)."""
    r = subprocess.run(["make", "-s", "--no-print-directory", "-C", PKG_DIR, "--eval", "lab-devflags: ; @echo $(DEVFLAGS)", "lab-devflags"],
                       check=True, capture_output=True, text=True)
    return r.stdout.split()


def build(force=False, contract="off"):
    """Compile the lab for gfx950 with the strict kernels' flags (contract "off") or the RT_FLAG_FAST variant's ("fast") into
    tests/tools/bin (on demand, like cubic_guard_lab.build)."""
    so = SO if contract == "off" else SO.replace(".so", f"_{contract}.so")
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        tmp = so + ".tmp"
        subprocess.run([hipcc] + devflags() + ["-ffp-contract=" + contract, "-shared", "-I" + HERE, SRC, "-o", tmp], check=True)
        os.replace(tmp, so)
    return so


_LIB = {}


def lib(pkg, contract="off"):
    """The lab, loaded after pkg.lib() (which loads torch's HIP runtime first: a second runtime in the process would see no device)."""
    if contract not in _LIB:
        pkg.lib()
        L = C.CDLL(build(contract=contract))
        vp = C.c_void_p
        L.lab_libm.argtypes = [C.c_int, vp, C.c_uint64, vp]
        L.lab_rays.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp]
        L.lab_guard.argtypes = [vp, C.c_uint64, vp]
        for f in (L.lab_libm, L.lab_rays, L.lab_guard):
            f.restype = C.c_int
        _LIB[contract] = L
    return _LIB[contract]


def _check(status, what):
    if status != 0:
        raise RuntimeError(f"{what}: HIP status {status}")


def device_libm(L, name, args):
    """The device's cbrt / acos / cos (the calls of solve_cubic) on float64 arguments."""
    x = np.ascontiguousarray(args, dtype=np.float64)
    y = np.empty_like(x)
    _check(L.lab_libm(FN[name], x.ctypes.data, len(x), y.ctypes.data), "lab_libm")
    return y


def device_rays(L, coefs, rays):
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    rays = np.ascontiguousarray(rays, dtype=RAY)
    out = np.zeros(len(rays), dtype=OUT)
    _check(L.lab_rays(coefs.ctypes.data, coefs.shape[0], rays.ctypes.data, len(rays), out.ctypes.data), "lab_rays")
    return out


def device_guard(L, cases):
    """cases [n, 10]: t3, t2, t1, t0, m3, m2, m1, m0, max_t, decide -> (ok [n] bool, t [n])."""
    cases = np.ascontiguousarray(cases, dtype=np.float64).reshape(-1, 10)
    out = np.empty((len(cases), 2), dtype=np.float64)
    _check(L.lab_guard(cases.ctypes.data, len(cases), out.ctypes.data), "lab_guard")
    return out[:, 0] != 0.0, out[:, 1]


# ---- the oracle's side (the CPU lab) ----
_CPU = None


def cpu_lib():
    global _CPU
    if _CPU is None:
        L = CPU.build()
        L.lab_enumerate.restype = C.c_uint64
        L.lab_enumerate.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_uint64]
        L.lab_oracle.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        _CPU = L
    return _CPU


def _cam(cam):
    return np.ascontiguousarray(O.IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)


def enumerate_rays(osc, cam=None):
    """Every degree-3 test of the frame (primary rays, shadow rays of their hits, first bounces of mirror hits): (RAY [n], WHERE [n])."""
    L, sc, cam = cpu_lib(), osc.c_scene(), _cam(cam)
    camp = cam.ctypes.data_as(C.POINTER(C.c_double))
    n = int(L.lab_enumerate(C.byref(sc), camp, None, None, 0))
    rays, where = np.zeros(n, dtype=RAY), np.zeros(n, dtype=WHERE)
    assert L.lab_enumerate(C.byref(sc), camp, rays.ctypes.data, where.ctypes.data, n) == n
    return rays, where


def oracle_rays(osc, rays):
    """The oracle's intersect_ray on each record, under whatever libm hook is active: (t, dense t3..t0 [n, 4], branch)."""
    sc, rays = osc.c_scene(), np.ascontiguousarray(rays, dtype=RAY)
    t, tc, br = np.empty(len(rays)), np.empty((len(rays), 4)), np.empty(len(rays), dtype=np.int32)
    cpu_lib().lab_oracle(C.byref(sc), rays.ctypes.data, len(rays), t.ctypes.data, tc.ctypes.data, br.ctypes.data)
    return t, tc, br


def evaluator(L):
    return lambda name, args: device_libm(L, name, args)


def oracle_rays_device_libm(L, osc, rays, libm=None):
    """oracle_rays with the device's cbrt / acos / cos in the solver.  Returns ((t, tc, branch), Libm, rounds)."""
    return O.under_libm(lambda: oracle_rays(osc, rays), evaluator(L), libm)


def render_device_libm(L, osc, cam=None, rows=None, counters=False, nthreads=8, libm=None):
    """The oracle's frame (or rows) with the device's cbrt / acos / cos in the solver: (render's result, Libm, rounds)."""
    return O.under_libm(lambda: osc.render(cam=cam, rows=rows, counters=counters, nthreads=nthreads), evaluator(L), libm)


def compare_device_libm(pkg, got, osc, cam=None, rows=None, nthreads=8):
    """A device frame (or rows, RGB) against the oracle under the device's libm: conftest.compare's dict, plus `bad` -- the (row, column)
    of every pixel beyond its bar (rows: indices into `got`) -- and the libm rounds it took."""
    from conftest import compare
    want, libm, rounds = render_device_libm(lib(pkg), osc, cam=cam, rows=rows, nthreads=nthreads)
    c = compare(got, want)
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    diff = np.abs(g - w)
    rel = diff / np.maximum(np.maximum(np.abs(g), np.abs(w)), 1e-300)
    c["bad"] = [tuple(int(v) for v in p) for p in np.argwhere(((rel > 1e-5) & (diff > 1e-7)).any(axis=-1))]
    c["not_identical_pixels"] = int((g != w).any(axis=-1).sum())
    c["libm_rounds"] = rounds
    return c


# ---- high-precision reference of the special functions ----
def _mp_func(name):
    import mpmath
    return {"cbrt": lambda x: mpmath.sign(x) * mpmath.cbrt(abs(x)), "acos": mpmath.acos, "cos": mpmath.cos}[name]


def ulp_error(name, args, values, dps=60):
    """|value - f(x)| in units of the last place of f(x) rounded to float64, per argument, f by mpmath at `dps` digits (so that 0.5 means
    correctly rounded).  Where f has no real value (acos beyond [-1, 1]) or x is not finite, the value must be NaN / the matching infinity
    (0) or it counts as inf."""
    import mpmath
    f = _mp_func(name)
    err = np.zeros(len(args))
    with mpmath.workdps(dps):
        for i, (x, y) in enumerate(zip(np.asarray(args, dtype=np.float64).tolist(), np.asarray(values, dtype=np.float64).tolist())):
            if not np.isfinite(x) or (name == "acos" and abs(x) > 1.0):
                want = x if (name == "cbrt" and not np.isnan(x)) else np.nan
                err[i] = 0.0 if (np.isnan(want) and np.isnan(y)) or want == y else np.inf
                continue
            exact = f(mpmath.mpf(x))
            r = float(exact)   # (correctly rounded)
            if r == 0.0:
                err[i] = 0.0 if y == 0.0 else np.inf
                continue
            err[i] = float(abs(mpmath.mpf(y) - exact)) / float(np.spacing(abs(r))) if np.isfinite(y) else np.inf
    return err


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as graft
    pkg = graft.load_package()
    L = lib(pkg)
    for name in sys.argv[1:] or ["clebsch", "cayley", "cubic", "dingdong", "monkey_saddle"]:
        osc = O.load_scene(os.path.join(ROOT, "scenes", name + ".yml")).with_size(200, 150)
        rays, where = enumerate_rays(osc)
        out = device_rays(L, osc.coefs, rays)
        (t, _, br), libm, rounds = oracle_rays_device_libm(L, osc, rays)
        dense = out["refused"] != 0
        print(f"{name}: tests {len(rays)}, refused {int(dense.sum())}, dense t not bitwise {int((t[dense].view(np.uint64) != out['t'][dense].view(np.uint64)).sum())}, "
              f"libm rounds {rounds}, arguments {len(libm)}", flush=True)


if __name__ == "__main__":
    main()
