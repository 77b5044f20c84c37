"""rt_set_scene without a GPU: the ABI (symbols, signatures, struct size, the refusals that come before a device is looked for), the
update.h adapter's entry point, the build rules the kernel stands under, and -- the check that rt_create's own output did not move by
one byte when its derivations moved into csrc/rt_scene_pack.hpp -- the header against the inline code it replaced."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from conftest import ROOT, scene_path

HEADER = os.path.join(ROOT, "include", "mi355rt.h")
CSRC = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")


def header_text():
    return re.sub(r"\s+", " ", open(HEADER).read())


def test_header_declares_the_documented_signatures():
    t = header_text()
    for decl in ("int rt_set_scene(rt_ctx *ctx, const rt_scene_update *dev, void *stream);",
                 "int rt_set_scene_host(rt_ctx *ctx, const rt_scene_update *host, void *stream);",
                 "int rt_set_scene_status(rt_ctx *ctx, uint64_t *applied, uint64_t *rejected, uint32_t *reason, uint32_t *index);",
                 "int rt_debug_scene_blob(rt_ctx *ctx, void *out, size_t cap, size_t *bytes);"):
        assert decl in t, decl
    m = re.search(r"typedef struct rt_scene_update \{(.*?)\} rt_scene_update;", t)
    fields = re.findall(r"const (double|float) \*(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == [("double", "coefs"), ("float", "reflection"), ("float", "albedo"), ("double", "light_p"), ("float", "light_color")]
    assert "#define RT_ABI_VERSION 3" in t


def test_symbols_exist_and_the_abi_version_stays(pkg):
    lib = pkg.lib()
    for name in ("rt_set_scene", "rt_set_scene_host", "rt_set_scene_status", "rt_debug_scene_blob"):
        assert hasattr(lib, name) and name in pkg.ABI_SYMBOLS, name
    assert lib.rt_abi_version() == 3


def test_struct_is_40_bytes(pkg, tmp_path):
    assert C.sizeof(pkg.SceneUpdate) == 40
    assert [f[0] for f in pkg.SceneUpdate._fields_] == ["coefs", "reflection", "albedo", "light_p", "light_color"]
    src = tmp_path / "size.c"
    src.write_text('#include "mi355rt.h"\n#include <stddef.h>\n_Static_assert(sizeof(rt_scene_update) == 40, "size");\n'
                   '_Static_assert(offsetof(rt_scene_update, light_color) == 32, "order");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")], check=True)


def test_null_context_and_null_struct_are_refused_without_a_device(pkg):
    lib = pkg.lib()
    u = pkg.SceneUpdate()
    fake_ctx = C.c_void_p(0)
    for fn in (lib.rt_set_scene, lib.rt_set_scene_host):
        assert fn(fake_ctx, C.byref(u), None) == -1
        assert b"null argument" in lib.rt_last_error()
    # a NULL struct is refused before the context is touched and before a device is looked for: any non-NULL handle will do
    handle = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    for fn in (lib.rt_set_scene, lib.rt_set_scene_host):
        assert fn(handle, None, None) == -1
        assert b"null argument" in lib.rt_last_error()
    assert lib.rt_set_scene_status(None, None, None, None, None) == -1
    n = C.c_size_t()
    assert lib.rt_debug_scene_blob(None, None, 0, C.byref(n)) == -1
    assert lib.rt_debug_scene_blob(handle, None, 0, None) == -1


def test_update_adapter_exports_the_scene_update(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.UPDATE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mi355rt_update_scene\b", out)


def test_update_adapter_refuses_before_init_update(pkg):
    upd = C.CDLL(pkg.UPDATE_LIB_PATH)
    upd.mi355rt_update_scene.argtypes = [C.c_void_p]
    sc = pkg.Scene.load_from_file(scene_path("20spheres"))
    assert upd.mi355rt_update_scene(sc._h) == -1 and b"no init_update() call yet" in pkg.lib().rt_last_error()


# ---- the shared header against the packing code rt_create had inline (tests/tools/scene_pack_lab.*) ---------------------------------
def lab():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import scene_pack_lab
    return scene_pack_lab


def assert_same_records(L, name, new, old):
    diff = np.flatnonzero(new != old)
    assert diff.size == 0, f"{name}: {diff.size} of {new.size} bytes differ from the inline packing code, the first at offset {diff[0]}"
    assert new.size > 16


def test_header_packs_the_raw_descriptor_scenes_as_the_inline_code_did():
    """Every named oddity (light vectors at EPS, NaN / inf colours and albedos, odd reflection ratios) and the random sample of
    tests/tools/raw_desc_scenes.py: DevObject, table entry, MatEntry, DevLight, LightK and the scene words, byte for byte."""
    L = lab()
    import raw_desc_scenes as R
    for name in sorted(R.NAMED):
        assert_same_records(L, name, *L.pack_scene(R.named(name)[0]))
    for seed in range(R.N_SEEDS):
        assert_same_records(L, f"seed {seed}", *L.pack_scene(R.scene(seed)[0]))


def test_header_packs_the_edge_inputs_as_the_inline_code_did(pkg):
    """The scenes and updates of tests/test_set_scene_gpu.py (radii near 0, -0.0 centres, an own-sphere window that overflows FP32,
    u2 just above EPS, a cubic), the rejected ones (r^2 <= 0, a NaN albedo, a zero light vector ...) and hand-made extremes."""
    L = lab()
    import test_set_scene_gpu as G
    cases = [(f"{key} base", G.base_scene(pkg, key)) for key in ("20spheres", "mixed", "cubic")]
    cases += [(f"{key} {which}", G.update_of(pkg, key, which)) for key, which in (("20spheres", "moved"), ("20spheres", "edges"), ("mixed", "moved"), ("cubic", "moved"))]
    cases += [(name, G.rejected_case(pkg, name)[1]) for name in ("sphere to ellipsoid", "r^2 <= 0", "plane gains a square term", "first mirror", "NaN albedo",
                                                                   "zero light direction", "cubic coefficient")]
    x = G.changed(G.base_scene(pkg, "20spheres"))
    for i, (c, r) in enumerate([((0, 0, 0), 5e-324 ** 0.5), ((1e150, 0, 0), 1.0), ((0, 0, 0), 1e160), ((0, 0, 0), 1.8e19), ((0, 0, 0), 1.9e19), ((3, 4, 12), 1e-160),
                                ((np.inf, 0, 0), 1.0), ((np.nan, 0, 0), 1.0), ((-0.0, -0.0, -0.0), 1.0), ((1e-300, 1e-300, 1e-300), 1e-150)]):
        x["coefs"][i] = G.sphere(c, r)
    x["coefs"][10][19] = np.nan
    x["coefs"][11][10] = np.nextafter(1.0, 2.0)   # not a unit sphere by one ulp
    x["reflection"][:4] = (1e-7, np.float32(1.0000001e-7), -0.0, np.nan)
    x["albedo"][2] = (np.inf, 0.0, -0.0)
    for i, p in enumerate([(0, 0, 0), (-0.0, 0, 0), (3.1622e-4, 0, 0), (3.1623e-4, 0, 0), (1e-30, 0, 0), (1e30, 1e30, 1e30), (3e38, 3e38, 0), (1e39, 0, 0), (np.nan, 1, 0),
                           (np.inf, -np.inf, 0), (1e-46, 0, 0)]):
        x["light_p"][i] = p
    x["light_color"][3] = (np.nan, 0, 0)
    cases.append(("extremes", x))
    for name, a in cases:
        assert_same_records(L, name, *L.pack_both(a["coefs"], a["reflection"], a["albedo"], a["light_is_spherical"], a["light_p"], a["light_color"]))


def test_kernel_is_built_without_contraction_and_under_the_no_spill_rule():
    mk = open(os.path.join(ROOT, "cuda-ray-tracer_amd", "Makefile")).read()
    rule = re.search(r"\$\(BUILD\)/csrc/rt_set_scene\.o:.*?\n\t@mkdir[^\n]*\n\t([^\n]*)", mk)
    assert rule and "-ffp-contract=off" in rule.group(1) and "-Rpass-analysis=kernel-resource-usage" in rule.group(1) and "$@.remarks" in rule.group(1)
    assert "$(BUILD)/csrc/rt_set_scene.o" in re.search(r"^OBJ\s*:=.*$", mk, flags=re.M).group(0)
    report = os.path.join(ROOT, "cuda-ray-tracer_amd", "build", "spills.txt")
    if os.path.exists(report):   # (written by this tree's Makefile; tests/test_abi.py holds the whole report to "no spill, no private segment")
        lines = [l for l in open(report).read().splitlines() if "set_scene_kernel" in l]
        assert lines and all(l.rstrip().endswith("scratch 0") and "VGPR spills   0" in l for l in lines), lines
