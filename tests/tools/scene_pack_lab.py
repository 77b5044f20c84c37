#!/usr/bin/env python3
"""Host lab behind csrc/rt_scene_pack.hpp: the header compiled for the host (tests/tools/scene_pack_lab.cpp, called the way rt_create
calls it) against the packing code rt_create had inline before the header existed (tests/tools/scene_pack_parent.cpp, a translation unit
of its own that never sees the header).  Both write every derived record of a scene -- DevObject, the class-table entry, MatEntry,
DevLight, LightK, and the scene words has_mirror / n_cullable / lights_plain -- and the records must agree byte for byte: own_lo /
own_hi, inv_r, len_u and s_*, which no image shows, included.  No GPU.
usage: python tests/tools/scene_pack_lab.py      (the raw-descriptor scenes of raw_desc_scenes.py; prints the number of scenes and bytes)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOOLS = os.path.join(ROOT, "tests", "tools")


class LabDesc(C.Structure):
    _fields_ = [("n_objects", C.c_uint32), ("n_lights", C.c_uint32), ("coefs", C.c_void_p), ("reflection", C.c_void_p), ("albedo", C.c_void_p),
                ("light_is_spherical", C.c_void_p), ("light_p", C.c_void_p), ("light_color", C.c_void_p)]


_LIB = None


def build():
    global _LIB
    if _LIB is None:
        out = os.path.join(TOOLS, "bin", "libscene_pack_lab.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # the flags of the library's own host code (cuda-ray-tracer_amd/Makefile, HOSTFLAGS): no FMA contraction
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + TOOLS, os.path.join(TOOLS, "scene_pack_lab.cpp"), os.path.join(TOOLS, "scene_image_lab.cpp"),
                        os.path.join(TOOLS, "scene_pack_parent.cpp"), "-o", out], check=True)
        lib = C.CDLL(out)
        lib.lab_pack_bytes.restype = C.c_uint64
        lib.lab_pack_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.lab_pack_header.argtypes = lib.lab_pack_parent.argtypes = [C.POINTER(LabDesc), C.c_void_p]
        lib.lab_pack_header.restype = lib.lab_pack_parent.restype = None
        lib.lab_scene_image.restype = C.c_uint64
        lib.lab_scene_image.argtypes = [C.POINTER(LabDesc), C.c_uint32, C.c_void_p, C.c_uint64]
        _LIB = lib
    return _LIB


def pack_both(coefs, reflection, albedo, light_is_spherical, light_p, light_color):
    """(bytes packed with rt_scene_pack.hpp, bytes packed with the inline code of old) for one scene's descriptor arrays."""
    lib = build()
    keep = [np.ascontiguousarray(coefs, np.float64), np.ascontiguousarray(reflection, np.float32), np.ascontiguousarray(albedo, np.float32),
            np.ascontiguousarray(light_is_spherical, np.uint8), np.ascontiguousarray(light_p, np.float64), np.ascontiguousarray(light_color, np.float32)]
    no, nl = keep[1].size, keep[3].size
    assert keep[0].size == 20 * no and keep[2].size == 3 * no and keep[4].size == 3 * nl and keep[5].size == 3 * nl
    d = LabDesc(no, nl, *[a.ctypes.data for a in keep])
    n = lib.lab_pack_bytes(no, nl)
    new, old = np.full(n, 0x5A, np.uint8), np.full(n, 0xC3, np.uint8)
    lib.lab_pack_header(C.byref(d), new.ctypes.data)
    lib.lab_pack_parent(C.byref(d), old.ctypes.data)
    return new, old


def scene_image(coefs, reflection, albedo, light_is_spherical, light_p, light_color, flags=0):
    """The scene image a context with these rt_config flags uploads, as rt_debug_scene_blob returns it: [blob][DevLight x n][LightK x n]."""
    lib = build()
    keep = [np.ascontiguousarray(coefs, np.float64), np.ascontiguousarray(reflection, np.float32), np.ascontiguousarray(albedo, np.float32),
            np.ascontiguousarray(light_is_spherical, np.uint8), np.ascontiguousarray(light_p, np.float64), np.ascontiguousarray(light_color, np.float32)]
    d = LabDesc(keep[1].size, keep[3].size, *[a.ctypes.data for a in keep])
    out = np.zeros(lib.lab_scene_image(C.byref(d), flags, None, 0), np.uint8)
    assert lib.lab_scene_image(C.byref(d), flags, out.ctypes.data, out.size) == out.size
    return out


def pack_scene(osc):
    """... for an oracle scene (raw_desc_scenes.py)."""
    return pack_both(osc.coefs, osc.reflection, osc.albedo, osc.light_is_spherical, osc.light_p, osc.light_color)


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TOOLS)
    import raw_desc_scenes as R
    scenes = [(name, R.named(name)[0]) for name in sorted(R.NAMED)] + [(f"seed {s}", R.scene(s)[0]) for s in range(R.N_SEEDS)]
    total = bad = 0
    for name, osc in scenes:
        new, old = pack_scene(osc)
        total += new.size
        if not np.array_equal(new, old):
            bad += 1
            print(f"{name}: {int((new != old).sum())} of {new.size} bytes differ, the first at {int(np.flatnonzero(new != old)[0])}")
    print(f"{len(scenes)} scenes, {total} bytes, {bad} scenes differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
