"""Device leg of tests/tools/cull_lab.py: tests/tools/cull_device_lab.hip evaluates the lab's records on the GPU, one record per lane.
Built at test time with DEVFLAGS of cuda-ray-tracer_amd/Makefile plus -ffp-contract=off (the strict kernels' flags), or plus
-ffp-contract=fast -DRT_FAST=1 (the FAST variant's), into tests/tools/bin."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG_DIR = os.path.join(ROOT, "cuda-ray-tracer_amd")
sys.path.insert(0, HERE)
import cull_lab as CPU  # noqa: E402

SRC = os.path.join(HERE, "cull_device_lab.hip")
DEPS = [SRC, os.path.join(HERE, "cull_lab_records.h"), os.path.join(PKG_DIR, "Makefile")] + \
       [os.path.join(PKG_DIR, "csrc", f) for f in ("rt_wavefront_math.hpp", "rt_math.hpp", "rt_scene_dev.h")]
KIND = {"cone": 0, "pyr": 1, "sh": 2, "us": 3, "gq": 4}
VARIANT = {"strict": ["-ffp-contract=off"], "fast": ["-DRT_FAST=1", "-ffp-contract=fast"]}


def devflags():
    """DEVFLAGS of cuda-ray-tracer_amd/Makefile, as make expands them."""
    r = subprocess.run(["make", "-s", "--no-print-directory", "-C", PKG_DIR, "--eval", "lab-devflags: ; @echo $(DEVFLAGS)", "lab-devflags"],
                       check=True, capture_output=True, text=True)
    return r.stdout.split()


def build(variant="strict", force=False):
    so = os.path.join(HERE, "bin", f"libcull_device_lab_{variant}.so")
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        tmp = so + ".tmp"
        subprocess.run([hipcc] + devflags() + VARIANT[variant] + ["-shared", "-I" + HERE, SRC, "-o", tmp], check=True)
        os.replace(tmp, so)
    return so


_LIBS = {}


def lib(pkg, variant="strict"):
    """The lab, loaded after pkg.lib() (which loads the HIP runtime the process is to use)."""
    if variant not in _LIBS:
        pkg.lib()
        L = C.CDLL(build(variant))
        L.lab_device_eval.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.lab_device_eval.restype = C.c_int
        _LIBS[variant] = L
    return _LIBS[variant]


def evaluate(L, kind, rec):
    """As cull_lab.evaluate, on the device: one launch over all records of this kind."""
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, CPU.REC[kind])
    v = np.full(len(rec), -1, dtype=np.int32)
    crec = np.zeros((len(rec), 6))
    status = L.lab_device_eval(KIND[kind], rec.ctypes.data, len(rec), v.ctypes.data, crec.ctypes.data if kind == "sh" else None)
    if status != 0:
        raise RuntimeError(f"lab_device_eval({kind}): HIP status {status}")
    return (v, crec) if kind == "sh" else v
