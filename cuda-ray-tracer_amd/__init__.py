"""Python host binding of the MI355X-native ray-tracing path (ctypes over the C ABI, include/mi355rt.h).

The directory name carries a hyphen (it mirrors the reference's repository name), so import it through
``__graft_entry__.load_package()`` which registers it as module ``cuda_ray_tracer_amd``.

Names follow the reference's host interface (include/update.h, include/scene.h):
``Scene.load_from_file``, ``Renderer`` = ``init_update`` / ``update`` / ``cleanup_update``.
There is NO CPU fallback: constructing a ``Renderer`` without a usable GPU raises ``RtError``.
PyTorch is optional plumbing here (device tensors can be handed in as raw pointers + a stream handle).
"""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355RT_LIB") or os.path.join(_HERE, "libmi355rt.so")   # MI355RT_LIB: another build of the same ABI, for A/B measurements
UPDATE_LIB_PATH = os.path.join(_HERE, "libmi355rt_update.so")
MULTI_LIB_PATH = os.path.join(_HERE, "libmi355rt_multi.so")   # several GPUs behind one call; the only library that links RCCL
DRIVER_PATH = os.path.join(os.path.dirname(_HERE), "tests", "host_driver", "update_driver")   # headless host of the update.h contract (tests)
PICK_DRIVER_PATH = os.path.join(os.path.dirname(_HERE), "tests", "host_driver", "pick_driver")   # ... and of mi355rt_update_pick
# what `make all` produces, the base library first (the one a caller checks for)
BUILD_PRODUCTS = (os.path.join(_HERE, "libmi355rt.so"), MULTI_LIB_PATH, UPDATE_LIB_PATH, DRIVER_PATH, PICK_DRIVER_PATH)

RT_NCOEF = 20
RT_FLAG_STRICT, RT_FLAG_FAST, RT_FLAG_COUNT, RT_FLAG_SIMPLE, RT_FLAG_NOCULL, RT_FLAG_STATIC_ORDER, RT_FLAG_NOSCAN, RT_FLAG_PLAIN_ORDER = 0, 1, 2, 4, 8, 16, 32, 64
RT_FLAG_NOSPLIT = 128
RT_FLAG_NOLEAN = 256
RT_FLAG_SSAA2, RT_FLAG_SSAA4 = 512, 1024   # k x k supersampling with an exact box-filter resolve (include/mi355rt.h)
RT_FLAG_SSAA_ADAPTIVE = 2048                # ... only where the plain frame shows contrast (with RT_FLAG_SSAA2 or RT_FLAG_SSAA4)
RT_FLAG_SSAA_GEOMETRY = 4096                # ... and where the primary hit changes object or its normal turns (with RT_FLAG_SSAA_ADAPTIVE)
RT_FLAG_STREAM = 8192                       # render with the streamed frame kernel whatever the scene's size (scenes too large for LDS take it anyway)
RT_FLAG_STREAM_QUERIES = 16384              # the query entry points take their streamed kernels where the context is streamed or the tables exceed LDS: no size refusal
RT_FLAG_STREAM_ADAPTIVE = 32768             # adaptive supersampling takes its streamed passes where the staged ones refuse the scene (or with RT_FLAG_STREAM): no size refusal
RT_FLAG_STREAM_CULL = 524288                # a streamed context keeps its unit spheres in a spatial order and culls them by 64-entry chunk (same frame)
RT_FLAG_STREAM_CULL_BOUNCE = 1048576        # ... and culls the chunks of its bounce rays per ray (with RT_FLAG_STREAM_CULL, mirrors and at least two chunks; same frame)
RT_FLAG_STREAM_CULL_RAYS = 2097152          # ... and culls the chunks per caller-supplied ray in the ray queries (with RT_FLAG_STREAM_CULL, streamed queries and at least two chunks; same outputs)
RT_FLAG_STREAM_CULL_PIXELS = 4194304        # ... and culls the chunks by the block's cone in the pixel queries (with RT_FLAG_STREAM_CULL, streamed queries and at least two chunks; same outputs)
RT_FLAG_STREAM_CULL_REORDER = 8388608       # ... and reorder_scene() puts the unit spheres back into that spatial order after set_scene moved them (with RT_FLAG_STREAM_CULL; same frame)
RT_FLAG_STREAM_CULL_GROUPS = 16777216       # ... and update() asks a second level of bounds first, one per 64 chunk bounds (with RT_FLAG_STREAM_CULL and at least two groups: 4 097 unit spheres; same frame)
SSAA_DEFAULT_THRESHOLD = 1.0 / 32.0
RT_FMT_RGBA32F, RT_FMT_RGBA8 = 0, 1
RT_ERR_NO_DEVICE = -4

# every symbol include/mi355rt.h declares (tests check the built library exports all of them)
ABI_SYMBOLS = [
    "rt_abi_version", "rt_last_error", "rt_set_last_error", "rt_scene_load_file", "rt_scene_new", "rt_scene_add_object",
    "rt_scene_add_light", "rt_surface_make", "rt_scene_set_size", "rt_scene_set_max_reflections",
    "rt_scene_get_desc", "rt_scene_free", "rt_camera_matrix", "rt_create", "rt_render", "rt_local_rows", "rt_max_local_rows",
    "rt_row_map", "rt_pixel_bytes", "rt_device_fb", "rt_download", "rt_assemble", "rt_assemble_planes", "rt_merge_object_extents", "rt_sparse_bytes", "rt_sparse_msg_bytes", "rt_render_sparse", "rt_pack_sparse", "rt_assemble_sparse", "rt_sparse_stamp_bytes",
    "rt_assemble_sparse_incremental",
    "rt_set_ssaa_threshold", "rt_set_ssaa_geometry", "rt_get_ssaa_refined", "rt_get_streamed", "rt_get_streamed_queries", "rt_get_streamed_adaptive",
    "rt_get_stream_cull", "rt_debug_stream_bounds", "rt_debug_stream_cull", "rt_get_stream_cull_adaptive", "rt_debug_stream_cull_adaptive",
    "rt_get_stream_cull_bounce", "rt_debug_stream_cull_bounce", "rt_get_stream_cull_rays", "rt_debug_stream_cull_rays",
    "rt_get_stream_cull_pixels", "rt_debug_stream_cull_pixels", "rt_get_stream_groups", "rt_debug_stream_groups", "rt_debug_stream_group_bounds",
    "rt_render_gbuffer", "rt_pick", "rt_object_extents", "rt_object_extents_host",
    "rt_trace_rays", "rt_occluded_rays", "rt_trace_rays_host", "rt_shade_rays", "rt_shade_rays_host",
    "rt_trace_paths", "rt_trace_paths_host", "rt_primary_rays", "rt_pick_paths",
    "rt_sort_rays_work_bytes", "rt_sort_rays", "rt_permute",
    "rt_set_scene", "rt_set_scene_host", "rt_set_scene_status", "rt_debug_scene_blob", "rt_reorder_scene", "rt_get_stream_cull_reorder",
    "rt_get_counters", "rt_get_counters_detail", "rt_debug_counters", "rt_debug_stamp_rows", "rt_debug_wave_box", "rt_destroy",
]
# ... and the ones libmi355rt_multi.so exports
MULTI_ABI_SYMBOLS = ["rt_create_multi", "rt_render_multi", "rt_multi_wait", "rt_multi_fb", "rt_multi_stream", "rt_multi_download", "rt_multi_info",
                     "rt_multi_last_transfer", "rt_multi_set_ssaa_threshold", "rt_multi_set_ssaa_geometry", "rt_multi_destroy",
                     "rt_set_scene_multi", "rt_reorder_scene_multi", "rt_multi_set_scene_status", "rt_multi_query_ctx", "rt_render_gbuffer_multi", "rt_object_extents_multi",
                     "rt_object_extents_multi_host"]
RT_MULTI_SELF_EXCHANGE = 0x10000
RT_MULTI_BANDWISE = 0x20000
RT_MULTI_SPARSE = 0x40000


class RtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"mi355rt error {code}: {message}")
        self.code = code
        self.message = message


class SceneException(RtError):
    """Scene description rejected -- what the reference reports as SceneException (scene-exception.h)."""


class SceneDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("vertical_fov", C.c_double),
                ("bg_color", C.c_float * 3), ("max_reflections", C.c_uint32),
                ("n_objects", C.c_uint32), ("n_lights", C.c_uint32),
                ("coefs", C.POINTER(C.c_double)), ("reflection", C.POINTER(C.c_float)),
                ("albedo", C.POINTER(C.c_float)), ("light_is_spherical", C.POINTER(C.c_uint8)),
                ("light_p", C.POINTER(C.c_double)), ("light_color", C.POINTER(C.c_float))]


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("rank", C.c_uint32), ("world", C.c_uint32), ("band_rows", C.c_uint32),
                ("flags", C.c_uint32), ("format", C.c_uint32)]


class CountersDetail(C.Structure):
    _fields_ = [("tests_executed", C.c_uint64 * 4), ("solves", C.c_uint64 * 3), ("cull_evals", C.c_uint64 * 5), ("cubic_branch", C.c_uint64 * 4),
                ("shadow_rays_traced", C.c_uint64), ("hit_lights_shaded", C.c_uint64), ("primary_rays_formed", C.c_uint64), ("cubic_points", C.c_uint64), ("cubic_refused", C.c_uint64)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("primary_rays", "shadow_rays", "reflect_rays", "tests", "hits", "solves", "tests_executed", "cull_evals")]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n, _ in self._fields_}
        d["rays_total"] = d["primary_rays"] + d["shadow_rays"] + d["reflect_rays"]
        return d


class Hit(C.Structure):
    """rt_hit (include/mi355rt.h): what lies under one pixel's primary ray; 48 bytes."""
    _fields_ = [("t", C.c_double), ("point", C.c_double * 3), ("normal", C.c_float * 3), ("object", C.c_int32)]


HIT_DTYPE = np.dtype([("t", np.float64), ("point", np.float64, 3), ("normal", np.float32, 3), ("object", np.int32)])   # the same record, for numpy


# rt_object_extent (include/mi355rt.h): per object, the pixels that show it, their box and their range of t; 40 bytes
EXTENT_DTYPE = np.dtype([("pixels", np.uint64), ("x_min", np.uint32), ("y_min", np.uint32), ("x_max", np.uint32), ("y_max", np.uint32),
                         ("t_min", np.float64), ("t_max", np.float64)])


class Ray(C.Structure):
    """rt_ray (include/mi355rt.h): origin and direction of one ray query, the direction used as given; 48 bytes."""
    _fields_ = [("o", C.c_double * 3), ("d", C.c_double * 3)]


RAY_DTYPE = np.dtype([("o", np.float64, 3), ("d", np.float64, 3)])   # the same record, for numpy


class PathEnd(C.Structure):
    """rt_path_end (include/mi355rt.h): how the path of one ray along its mirror bounces ended; 16 bytes."""
    _fields_ = [("segments", C.c_uint32), ("end", C.c_uint32), ("ratio", C.c_float), ("object", C.c_int32)]


PATH_END_DTYPE = np.dtype([("segments", np.uint32), ("end", np.uint32), ("ratio", np.float32), ("object", np.int32)])   # the same record, for numpy
RT_PATH_MISS, RT_PATH_SURFACE, RT_PATH_ESCAPED, RT_PATH_CAP = 0, 1, 2, 3
RT_PATH_MAX_SEGMENTS = 64


class SceneUpdate(C.Structure):
    """rt_scene_update (include/mi355rt.h): five raw descriptor arrays, any of them NULL = keep what the context holds; 40 bytes."""
    _fields_ = [("coefs", C.c_void_p), ("reflection", C.c_void_p), ("albedo", C.c_void_p), ("light_p", C.c_void_p), ("light_color", C.c_void_p)]


SCENE_UPDATE_FIELDS = (("coefs", np.float64), ("reflection", np.float32), ("albedo", np.float32), ("light_p", np.float64), ("light_color", np.float32))
RT_SCENE_REJECT_CLASS, RT_SCENE_REJECT_BOUND, RT_SCENE_REJECT_MIRROR, RT_SCENE_REJECT_CUBIC, RT_SCENE_REJECT_LIGHT = 1, 2, 3, 4, 5


def build(verbose=False):
    """Compile libmi355rt.so / libmi355rt_update.so in-tree for gfx950 (hipcc cross-compiles without a GPU).  Builds from several
    processes at once take turns (a lock file in build/): each waits for the one in progress, whose products it then finds up to date."""
    os.makedirs(os.path.join(_HERE, "build"), exist_ok=True)
    with open(os.path.join(_HERE, "build", ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-C", _HERE, "-j4", "all"], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:])
        print(r.stderr[-4000:])
    if r.returncode != 0:
        raise RuntimeError("building libmi355rt.so failed")
    return LIB_PATH


_lib = None


def lib():
    """The loaded C-ABI library.  Fails loudly when it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RtError(-3, f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        # PyTorch-ROCm ships its own libamdhip64; if it is going to be used in this process (device tensors,
        # torch.distributed) it must be the copy that gets loaded, so load it BEFORE our library pulls in the
        # system one -- two different HIP runtimes in one process leave the second without devices.
        try:
            import torch  # noqa: F401
        except Exception:  # torch is plumbing, not a requirement of the C ABI
            pass
        L = C.CDLL(LIB_PATH)
        vp, dp, fp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float)
        L.rt_abi_version.restype = C.c_int
        if (L.rt_abi_version() & 0x4000) and not os.environ.get("MI355RT_ALLOW_DIAGNOSTIC"):
            raise RtError(-3, f"{LIB_PATH} is a diagnostic build (make STAMPS=1 / DEBUG_EXITS=1 / SPILLS_OK=1 ...), not the product: rebuild with plain "
                              "`make`, or set MI355RT_ALLOW_DIAGNOSTIC=1 for a measurement")
        L.rt_last_error.restype = C.c_char_p
        L.rt_scene_load_file.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.rt_scene_new.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, fp, C.POINTER(vp)]
        L.rt_scene_add_object.argtypes = [vp, dp, C.c_float, fp]
        L.rt_scene_add_light.argtypes = [vp, C.c_int, C.c_float, dp, fp]
        L.rt_surface_make.argtypes = [C.c_int, dp, dp, dp]
        L.rt_scene_set_size.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.rt_scene_set_max_reflections.argtypes = [vp, C.c_uint32]
        L.rt_scene_get_desc.argtypes = [vp, C.POINTER(SceneDesc)]
        L.rt_scene_free.argtypes = [vp]
        L.rt_scene_free.restype = None
        L.rt_camera_matrix.argtypes = [dp, C.c_double, C.c_double, dp]
        L.rt_create.argtypes = [C.POINTER(vp), C.POINTER(SceneDesc), C.POINTER(Config)]
        L.rt_render.argtypes = [vp, dp, vp, vp, fp]
        L.rt_local_rows.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_max_local_rows.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_row_map.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_pixel_bytes.argtypes = [vp]
        L.rt_pixel_bytes.restype = C.c_size_t
        L.rt_device_fb.argtypes = [vp]
        L.rt_device_fb.restype = vp
        L.rt_download.argtypes = [vp, vp, C.c_size_t]
        L.rt_assemble.argtypes = [vp, vp, vp, vp]
        L.rt_sparse_bytes.argtypes = [C.c_uint32]
        L.rt_sparse_bytes.restype = C.c_size_t
        L.rt_sparse_msg_bytes.argtypes = [C.c_uint32, C.c_uint32]
        L.rt_sparse_msg_bytes.restype = C.c_size_t
        L.rt_pack_sparse.argtypes = [vp, vp, vp, C.c_uint32, vp]
        L.rt_render_sparse.argtypes = [vp, dp, vp, C.c_uint32, vp, fp]
        L.rt_assemble_sparse.argtypes = [vp, vp, C.c_uint32, vp, vp]
        L.rt_sparse_stamp_bytes.argtypes = [vp]
        L.rt_sparse_stamp_bytes.restype = C.c_size_t
        L.rt_assemble_sparse_incremental.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp]
        L.rt_get_counters.argtypes = [vp, C.POINTER(Counters)]
        L.rt_get_counters_detail.argtypes = [vp, C.POINTER(CountersDetail)]
        L.rt_debug_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_debug_stamp_rows.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.rt_debug_wave_box.argtypes = [vp, dp, C.POINTER(C.c_uint64), C.c_uint32, fp]
        L.rt_destroy.argtypes = [vp]
        L.rt_set_ssaa_threshold.argtypes = [vp, C.c_float]
        L.rt_set_ssaa_geometry.argtypes = [vp, C.c_float]
        L.rt_get_ssaa_refined.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_get_streamed.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_get_streamed_queries.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_get_streamed_adaptive.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_get_stream_cull.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_debug_stream_bounds.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.rt_debug_stream_cull.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_get_stream_cull_adaptive.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_debug_stream_cull_adaptive.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_get_stream_cull_bounce.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_debug_stream_cull_bounce.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.rt_get_stream_cull_rays.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_debug_stream_cull_rays.argtypes = [vp, C.POINTER(C.c_uint64)]
        if LIB_PATH != os.environ.get("MI355RT_LIB") or hasattr(L, "rt_get_stream_cull_pixels"):   # (an earlier build under MI355RT_LIB: as rt_sort_rays below)
            L.rt_get_stream_cull_pixels.argtypes = [vp, C.POINTER(C.c_uint32)]
            L.rt_debug_stream_cull_pixels.argtypes = [vp, C.POINTER(C.c_uint64)]
        if LIB_PATH != os.environ.get("MI355RT_LIB") or hasattr(L, "rt_get_stream_groups"):   # (an earlier build under MI355RT_LIB: as rt_sort_rays below)
            L.rt_get_stream_groups.argtypes = [vp, C.POINTER(C.c_uint32)]
            L.rt_debug_stream_groups.argtypes = [vp, C.POINTER(C.c_uint64)]
            L.rt_debug_stream_group_bounds.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.rt_render_gbuffer.argtypes = [vp, dp, vp, vp, vp, vp, fp]
        L.rt_pick.argtypes = [vp, dp, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(Hit), vp]
        L.rt_object_extents.argtypes = [vp, dp, C.POINTER(C.c_uint32), vp, vp, fp]
        L.rt_object_extents_host.argtypes = [vp, dp, C.POINTER(C.c_uint32), vp, vp]
        L.rt_trace_rays.argtypes = [vp, vp, C.c_uint32, vp, vp, fp]
        L.rt_occluded_rays.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, fp]
        L.rt_trace_rays_host.argtypes = [vp, C.POINTER(Ray), C.c_uint32, C.POINTER(Hit), vp]
        L.rt_shade_rays.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, fp]
        L.rt_shade_rays_host.argtypes = [vp, C.POINTER(Ray), C.c_uint32, fp, vp]
        L.rt_trace_paths.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, fp]
        L.rt_trace_paths_host.argtypes = [vp, C.POINTER(Ray), C.c_uint32, C.c_uint32, C.POINTER(Hit), C.POINTER(Hit), C.POINTER(PathEnd), vp]
        L.rt_primary_rays.argtypes = [vp, dp, C.POINTER(C.c_uint32), vp, vp, fp]
        L.rt_pick_paths.argtypes = [vp, dp, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(Hit), C.POINTER(PathEnd), vp]
        L.rt_set_scene.argtypes = [vp, C.POINTER(SceneUpdate), vp]
        L.rt_set_scene_host.argtypes = [vp, C.POINTER(SceneUpdate), vp]
        L.rt_set_scene_status.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.rt_debug_scene_blob.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        if LIB_PATH != os.environ.get("MI355RT_LIB") or hasattr(L, "rt_reorder_scene"):   # (an earlier build under MI355RT_LIB: as rt_sort_rays below)
            L.rt_reorder_scene.argtypes = [vp, vp]
            L.rt_get_stream_cull_reorder.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.rt_assemble_planes.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, vp]
        L.rt_merge_object_extents.argtypes = [vp, vp, C.c_uint32, vp, vp]
        if LIB_PATH != os.environ.get("MI355RT_LIB") or hasattr(L, "rt_sort_rays"):   # (an earlier build of this ABI under MI355RT_LIB: calling them raises)
            L.rt_sort_rays_work_bytes.argtypes = [C.c_uint32]
            L.rt_sort_rays_work_bytes.restype = C.c_size_t
            L.rt_sort_rays.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_size_t, vp, fp]
            L.rt_permute.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_int, vp, fp]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        msg = lib().rt_last_error().decode("utf-8", "replace")
        raise (SceneException if rc == -2 else RtError)(rc, msg)


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


IDENTITY = np.eye(4, dtype=np.float64).reshape(16).copy()

_mlib = None


def multi_lib():
    """libmi355rt_multi.so (rt_create_multi / rt_render_multi ...).  Loaded on demand: it links RCCL."""
    global _mlib
    if _mlib is None:
        lib()   # the base library (and torch's HIP runtime, if torch is around) first
        if not os.path.exists(MULTI_LIB_PATH):
            raise RtError(-3, f"{MULTI_LIB_PATH} is missing: run __graft_entry__.build()")
        M = C.CDLL(MULTI_LIB_PATH)
        vp = C.c_void_p
        M.rt_create_multi.argtypes = [C.POINTER(vp), C.POINTER(SceneDesc), C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        M.rt_render_multi.argtypes = [vp, C.POINTER(C.c_double), vp, C.POINTER(C.c_float)]
        M.rt_multi_wait.argtypes = [vp]
        M.rt_multi_fb.argtypes = [vp]
        M.rt_multi_fb.restype = vp
        M.rt_multi_stream.argtypes = [vp]
        M.rt_multi_stream.restype = vp
        M.rt_multi_download.argtypes = [vp, vp, C.c_size_t]
        M.rt_multi_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        M.rt_multi_last_transfer.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        M.rt_multi_destroy.argtypes = [vp]
        M.rt_multi_set_ssaa_threshold.argtypes = [vp, C.c_float]
        M.rt_multi_set_ssaa_geometry.argtypes = [vp, C.c_float]
        M.rt_set_scene_multi.argtypes = [vp, C.POINTER(SceneUpdate)]
        M.rt_reorder_scene_multi.argtypes = [vp]
        M.rt_multi_set_scene_status.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        M.rt_multi_query_ctx.argtypes = [vp]
        M.rt_multi_query_ctx.restype = vp
        M.rt_render_gbuffer_multi.argtypes = [vp, C.POINTER(C.c_double), vp, vp, vp, C.POINTER(C.c_float)]
        M.rt_object_extents_multi.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32), vp, C.POINTER(C.c_float)]
        M.rt_object_extents_multi_host.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32), vp]
        _mlib = M
    return _mlib


class Scene:
    """Handle on a scene owned by the library (rt_scene).  Mirrors the reference's Scene (scene.h:17-36)."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    @staticmethod
    def load_from_file(path):
        h = C.c_void_p()
        _check(lib().rt_scene_load_file(os.fsencode(path), C.byref(h)))
        return Scene(h.value)

    @staticmethod
    def new(width, height, fov_deg, max_reflections=5, bg_color=(1.0, 1.0, 1.0)):
        h = C.c_void_p()
        bg = np.asarray(bg_color, dtype=np.float32)
        _check(lib().rt_scene_new(int(width), int(height), float(fov_deg), int(max_reflections), _fptr(bg), C.byref(h)))
        return Scene(h.value)

    def add_object(self, coefs, color, reflection_ratio=0.0):
        c = np.ascontiguousarray(coefs, dtype=np.float64)
        assert c.size == RT_NCOEF
        col = np.asarray(color, dtype=np.float32)
        _check(lib().rt_scene_add_object(self._h, _dptr(c), float(reflection_ratio), _fptr(col)))

    def add_light(self, kind, v, color=(1.0, 1.0, 1.0), intensity=1.0):
        vv = np.asarray(v, dtype=np.float64)
        col = np.asarray(color, dtype=np.float32)
        _check(lib().rt_scene_add_light(self._h, 1 if kind == "spherical" else 0, float(intensity), _dptr(vv), _fptr(col)))

    def set_size(self, width, height):
        _check(lib().rt_scene_set_size(self._h, int(width), int(height)))
        return self

    def set_max_reflections(self, n):
        _check(lib().rt_scene_set_max_reflections(self._h, int(n)))
        return self

    def desc(self):
        d = SceneDesc()
        _check(lib().rt_scene_get_desc(self._h, C.byref(d)))
        return d

    def arrays(self):
        """Copies of the flat scene arrays (for tests)."""
        d = self.desc()
        no, nl = d.n_objects, d.n_lights

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt).copy() if n else np.zeros(0, dt)
        return dict(width=d.width, height=d.height, vertical_fov=d.vertical_fov, bg_color=np.array(list(d.bg_color), np.float32),
                    max_reflections=d.max_reflections,
                    coefs=arr(d.coefs, no * RT_NCOEF, np.float64).reshape(no, RT_NCOEF), reflection=arr(d.reflection, no, np.float32),
                    albedo=arr(d.albedo, no * 3, np.float32).reshape(no, 3), light_is_spherical=arr(d.light_is_spherical, nl, np.uint8),
                    light_p=arr(d.light_p, nl * 3, np.float64).reshape(nl, 3), light_color=arr(d.light_color, nl * 3, np.float32).reshape(nl, 3))

    def close(self):
        if self._h:
            lib().rt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_matrix(pos=(0.0, 0.0, 0.0), yaw_deg=90.0, pitch_deg=0.0):
    """The reference host's camera_matrix() (src/ray-tracer.cpp:44-58) for a pose; 16 doubles, column-major."""
    p = np.asarray(pos, dtype=np.float64)
    out = np.empty(16, dtype=np.float64)
    _check(lib().rt_camera_matrix(_dptr(p), float(yaw_deg), float(pitch_deg), _dptr(out)))
    return out


def surface_make(kind, a=None, b=None):
    names = {"sphere": 0, "plane": 1, "dingDong": 2, "clebsch": 3, "cayley": 4}
    out = np.zeros(RT_NCOEF, dtype=np.float64)
    aa = np.asarray(a if a is not None else [0, 0, 0], dtype=np.float64)
    bb = np.asarray(b if b is not None else [0, 0, 0], dtype=np.float64)
    if bb.size == 1:
        bb = np.array([float(bb.reshape(-1)[0]), 0.0, 0.0])
    _check(lib().rt_surface_make(names[kind], _dptr(aa), _dptr(bb), _dptr(out)))
    return out


def desc_from_arrays(width, height, vertical_fov, bg_color, max_reflections, coefs, reflection, albedo,
                     light_is_spherical, light_p, light_color):
    """Build an rt_scene_desc from numpy arrays (kept alive on the returned object)."""
    keep = dict(coefs=np.ascontiguousarray(coefs, np.float64), reflection=np.ascontiguousarray(reflection, np.float32),
                albedo=np.ascontiguousarray(albedo, np.float32), kind=np.ascontiguousarray(light_is_spherical, np.uint8),
                light_p=np.ascontiguousarray(light_p, np.float64), light_color=np.ascontiguousarray(light_color, np.float32))
    d = SceneDesc()
    d.width, d.height, d.vertical_fov, d.max_reflections = int(width), int(height), float(vertical_fov), int(max_reflections)
    for i in range(3):
        d.bg_color[i] = float(bg_color[i])
    d.n_objects, d.n_lights = keep["reflection"].size, keep["kind"].size
    d.coefs, d.reflection, d.albedo = _dptr(keep["coefs"]), _fptr(keep["reflection"]), _fptr(keep["albedo"])
    d.light_is_spherical = keep["kind"].ctypes.data_as(C.POINTER(C.c_uint8))
    d.light_p, d.light_color = _dptr(keep["light_p"]), _fptr(keep["light_color"])
    d._keep = keep
    return d


from .sharding import (band_rows_of_rank, max_local_rows, assemble_index, gather_to_root, assemble_torch, sparse_words, bg_rgba8,  # noqa: E402,F401
                       bg_rgba32f, pack_sparse_numpy, assemble_sparse_numpy)


class _SortedRays:
    """What the sort=True keywords share: the rays uploaded and sorted on the device (rt_sort_rays), buffers on that device, gathers into
    the sorted order and scatters back into the caller's (rt_permute).  Everything is enqueued on `stream` (None: the default stream);
    sync() waits for it."""

    def __init__(self, r, rays, stream, keys=False):
        import torch
        self.r, self.n, self.stream = r, len(rays), stream
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self._torch = torch
        if self.n == 0:
            raise RtError(-1, "rt_sort_rays: n is 0")
        d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.float64).reshape(-1, 6)).to(self.dev)
        self.sorted = torch.empty((self.n, 6), dtype=torch.float64, device=self.dev)
        self.perm = torch.empty((self.n,), dtype=torch.int32, device=self.dev)
        self.keys = torch.empty((self.n,), dtype=torch.int32, device=self.dev) if keys else None
        nbytes = r.sort_work_bytes(self.n)
        work = torch.empty((nbytes,), dtype=torch.uint8, device=self.dev)
        torch.cuda.current_stream().synchronize()   # the upload ran on torch's current stream
        self._t0, self._t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self._t0.record(self._ext())
        r.sort_rays_into(d_rays.data_ptr(), self.n, self.sorted.data_ptr(), self.perm.data_ptr(), None if self.keys is None else self.keys.data_ptr(),
                         work.data_ptr(), nbytes, stream=stream, timed=False)
        self._keep = [d_rays, work]
        self.sorted_ptr = self.sorted.data_ptr()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.sync()
        self._keep = []
        return False

    def _ext(self):
        return self._torch.cuda.ExternalStream(self.stream) if self.stream else self._torch.cuda.default_stream()

    def sync(self):
        self._ext().synchronize()

    def result(self, shape, dtype):
        return self._torch.empty(shape, dtype=getattr(self._torch, dtype), device=self.dev)

    def gathered(self, host, elem_bytes):
        """A host array of one record per ray, on the device in the sorted order."""
        src = self._torch.from_numpy(host).to(self.dev)
        self._torch.cuda.current_stream().synchronize()
        dst = self._torch.empty_like(src)
        self.r.permute_into(self.perm.data_ptr(), self.n, src.data_ptr(), dst.data_ptr(), elem_bytes, stream=self.stream, timed=False)
        self._keep.append(src)
        return dst

    def scattered(self, t, elem_bytes, planes=1):
        """A device tensor of planes x n records in the sorted order, back in the caller's order (waits for it)."""
        out = self._torch.empty_like(t)
        self.r.permute_into(self.perm.data_ptr(), self.n, t.data_ptr(), out.data_ptr(), elem_bytes, planes=planes, scatter=True, stream=self.stream, timed=False)
        self._t1.record(self._ext())
        self.sync()
        return out

    def elapsed(self):
        return self._t0.elapsed_time(self._t1)


class Renderer:
    """init_update / update / cleanup_update (reference include/update.h:6-8) as an object."""

    def __init__(self, scene, device=-1, rank=0, world=1, band_rows=8, flags=RT_FLAG_STRICT, fmt=RT_FMT_RGBA32F, ssaa_threshold=None, ssaa_min_cos=None):
        self._h = None
        d = scene.desc() if isinstance(scene, Scene) else scene
        self._desc = d
        cfg = Config(int(device), int(rank), int(world), int(band_rows), int(flags), int(fmt))
        h = C.c_void_p()
        _check(lib().rt_create(C.byref(h), C.byref(d), C.byref(cfg)))
        self._h = h
        self.width, self.height = d.width, d.height   # the output frame (with supersampling too)
        self.fmt = fmt
        self.flags = int(flags)
        n = C.c_uint32()
        _check(lib().rt_local_rows(self._h, C.byref(n)))
        self.local_rows = n.value
        _check(lib().rt_max_local_rows(self._h, C.byref(n)))
        self.max_local_rows = n.value
        self.pixel_bytes = lib().rt_pixel_bytes(self._h)
        if ssaa_threshold is not None:
            self.set_ssaa_threshold(ssaa_threshold)
        if ssaa_min_cos is not None:
            self.set_ssaa_geometry(ssaa_min_cos)

    def set_ssaa_threshold(self, tau):
        """RT_FLAG_SSAA_ADAPTIVE: refine pixels whose 3x3 neighbourhood differs by more than tau in some channel (tau < 0: every
        pixel).  Applies from the next update(); a captured graph keeps the tau it was captured with."""
        _check(lib().rt_set_ssaa_threshold(self._h, float(tau)))

    def set_ssaa_geometry(self, min_cos):
        """RT_FLAG_SSAA_GEOMETRY: also refine pixels with an 8-neighbour on the same object whose normal makes a cosine below min_cos
        with theirs (-inf, the default: object boundaries only).  Applies from the next update(), like set_ssaa_threshold."""
        _check(lib().rt_set_ssaa_geometry(self._h, float(min_cos)))

    @property
    def refined(self):
        """RT_FLAG_SSAA_ADAPTIVE: the number of refined pixels of the last frame (waits for it)."""
        n = C.c_uint64()
        _check(lib().rt_get_ssaa_refined(self._h, C.byref(n)))
        return n.value

    @property
    def streamed(self):
        """True where update() is the streamed frame kernel: RT_FLAG_STREAM, or a scene whose tables do not fit a workgroup's LDS."""
        n = C.c_uint32()
        _check(lib().rt_get_streamed(self._h, C.byref(n)))
        return bool(n.value)

    @property
    def streamed_queries(self):
        """True where the queries (gbuffer, pick, object_extents, trace, occluded, shade, paths) are the streamed kernels:
        RT_FLAG_STREAM_QUERIES on a streamed context or on a scene whose class tables do not fit a workgroup's LDS."""
        n = C.c_uint32()
        _check(lib().rt_get_streamed_queries(self._h, C.byref(n)))
        return bool(n.value)

    @property
    def streamed_adaptive(self):
        """True where the halo, G and refine passes of an adaptive frame are the streamed kernels: RT_FLAG_STREAM_ADAPTIVE on an adaptive
        context that is created with RT_FLAG_STREAM or whose scene the staged passes cannot hold in a workgroup's LDS."""
        n = C.c_uint32()
        _check(lib().rt_get_streamed_adaptive(self._h, C.byref(n)))
        return bool(n.value)

    def stream_bounds(self):
        """Diagnostics: the chunk-bound table as the device holds it, as bytes (64 per chunk; rt_debug_stream_bounds; waits).  Empty
        where stream_cull is False."""
        n = C.c_size_t()
        _check(lib().rt_debug_stream_bounds(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            _check(lib().rt_debug_stream_bounds(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(n)))
        return out

    @property
    def stream_groups(self):
        """True where update() asks a second level of bounds, one per 64 chunk bounds, before the chunk bounds: RT_FLAG_STREAM_CULL_GROUPS
        on a context whose stream_cull is True, with at least two groups (4 097 unit spheres; rt_get_stream_groups)."""
        n = C.c_uint32()
        _check(lib().rt_get_stream_groups(self._h, C.byref(n)))
        return bool(n.value)

    def debug_stream_groups(self):
        """The eight group work words since the context was created (rt_debug_stream_groups; waits).  They exist only where stream_groups
        is True and MI355RT_STREAM_CULL_STATS=1 was in the environment when the context was created."""
        w = (C.c_uint64 * 8)()
        _check(lib().rt_debug_stream_groups(self._h, w))
        return [int(v) for v in w]

    def debug_stream_group_bounds(self):
        """Diagnostics: the group-bound table as the device holds it, as bytes (64 per group of 64 chunks; rt_debug_stream_group_bounds;
        waits).  Empty where stream_groups is False."""
        n = C.c_size_t()
        _check(lib().rt_debug_stream_group_bounds(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            _check(lib().rt_debug_stream_group_bounds(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(n)))
        return out

    @property
    def samples(self):
        """Supersampling factor k per axis: 1, 2 (RT_FLAG_SSAA2) or 4 (RT_FLAG_SSAA4)."""
        return 4 if self.flags & RT_FLAG_SSAA4 else (2 if self.flags & RT_FLAG_SSAA2 else 1)

    # init_update is the constructor; these two complete the reference's trio
    def update(self, cam=None, dev_fb=None, stream=None, timed=True):
        """Render one frame; returns device milliseconds (what the reference's update() returns) or None."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        ms = C.c_float(0.0)
        _check(lib().rt_render(self._h, _dptr(cam), C.c_void_p(dev_fb) if dev_fb else None,
                               C.c_void_p(stream) if stream else None, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def gbuffer(self, cam=None, object=True, t=True, normal=True, stream=None, timed=True):
        """The primary-hit G-buffer of this rank's rows (rt_render_gbuffer): torch device tensors (object int32 [rows, W], t float64
        [rows, W], normal float32 [rows, W, 4]; None for a plane not asked for) and the device milliseconds of the pass (None unless
        timed).  Misses: object -1, t +inf, normal 0."""
        import torch
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        dev = torch.device("cuda", torch.cuda.current_device())
        rows, w = self.local_rows, self.width
        po = torch.empty((rows, w), dtype=torch.int32, device=dev) if object else None
        pt = torch.empty((rows, w), dtype=torch.float64, device=dev) if t else None
        pn = torch.empty((rows, w, 4), dtype=torch.float32, device=dev) if normal else None
        ms = self.gbuffer_into(cam, po.data_ptr() if object else None, pt.data_ptr() if t else None, pn.data_ptr() if normal else None, stream=stream, timed=timed)
        return po, pt, pn, ms

    def gbuffer_into(self, cam, object_ptr, t_ptr, normal_ptr, stream=None, timed=True):
        """rt_render_gbuffer into the caller's device memory (raw pointers, None = plane not written)."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        ms = C.c_float(0.0)
        _check(lib().rt_render_gbuffer(self._h, _dptr(cam), C.c_void_p(object_ptr) if object_ptr else None, C.c_void_p(t_ptr) if t_ptr else None,
                                       C.c_void_p(normal_ptr) if normal_ptr else None, C.c_void_p(stream) if stream else None, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def pick(self, xy, cam=None, stream=None):
        """What lies under the pixels xy = [(x, y), ...] (global coordinates, row 0 = bottom): a structured numpy array of HIT_DTYPE
        records (t, point, normal, object), one per pixel (rt_pick; blocks)."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        q = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros(q.shape[0], dtype=HIT_DTYPE)
        _check(lib().rt_pick(self._h, _dptr(cam), q.ctypes.data_as(C.POINTER(C.c_uint32)), q.shape[0], out.ctypes.data_as(C.POINTER(Hit)),
                             C.c_void_p(stream) if stream else None))
        return out

    @staticmethod
    def _rect(rect):
        if rect is None:
            return None, None
        r = np.ascontiguousarray(rect, dtype=np.uint32).reshape(4)
        return r, r.ctypes.data_as(C.POINTER(C.c_uint32))

    def object_extents(self, cam=None, rect=None, stream=None):
        """Per object: how many pixels of rect = (x0, y0, x1, y1) (inclusive, global coordinates, row 0 = bottom; None = the whole
        frame) in this rank's rows show it, their bounding box and their range of t: a structured numpy array of n_objects EXTENT_DTYPE
        records (rt_object_extents_host; blocks).  An object that is not seen has pixels 0, x_min = y_min = 0xFFFFFFFF, x_max = y_max
        = 0, t_min +inf, t_max 0, so the records of several ranks merge by sum / min / max."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        keep, rp = self._rect(rect)
        out = np.zeros(self._desc.n_objects, dtype=EXTENT_DTYPE)
        buf = out if len(out) else np.zeros(1, dtype=EXTENT_DTYPE)   # (a scene without objects: the call still wants a pointer)
        _check(lib().rt_object_extents_host(self._h, _dptr(cam), rp, buf.ctypes.data_as(C.c_void_p), C.c_void_p(stream) if stream else None))
        return out

    def object_extents_into(self, cam, rect, out_ptr, stream=None, timed=True):
        """rt_object_extents into the caller's device memory (a raw pointer to n_objects records of 40 bytes, 8-byte aligned): device
        milliseconds, or None unless timed (then the call only enqueues two kernels and can be captured into a graph)."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        keep, rp = self._rect(rect)
        ms = C.c_float(0.0)
        _check(lib().rt_object_extents(self._h, _dptr(cam), rp, C.c_void_p(out_ptr) if out_ptr else None, C.c_void_p(stream) if stream else None,
                                       C.byref(ms) if timed else None))
        return ms.value if timed else None

    @staticmethod
    def rays(origins, dirs):
        """RAY_DTYPE records from origins and directions ([n, 3] each, or one of them a single vector for all rays)."""
        o, d = np.asarray(origins, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
        n = max(o.size, d.size) // 3
        out = np.zeros(n, dtype=RAY_DTYPE)
        out["o"] = o.reshape(-1, 3)
        out["d"] = d.reshape(-1, 3)
        return out

    def trace(self, origins, dirs, stream=None, sort=False):
        """The closest hit of every ray (rt_trace_rays_host; blocks): a structured numpy array of HIT_DTYPE records.  Directions are
        used as given (t is in units of |d|); a miss is object -1, t +inf, point and normal 0.  Works in every context kind.
        sort=True: the same records by way of rt_sort_rays -- the rays are sorted on the device, traced in that order and the hits
        scattered back (worth it for rays in no useful order on an RT_FLAG_STREAM_CULL_RAYS context)."""
        rays = self.rays(origins, dirs)
        if sort:
            with self._sorted(rays, stream) as q:
                hits = q.result((q.n, 6), "float64")
                self.trace_into(q.sorted_ptr, q.n, hits.data_ptr(), stream=stream, timed=False)
                return q.scattered(hits, 48).cpu().numpy().view(HIT_DTYPE).reshape(-1)
        out = np.zeros(len(rays), dtype=HIT_DTYPE)
        _check(lib().rt_trace_rays_host(self._h, rays.ctypes.data_as(C.POINTER(Ray)), len(rays), out.ctypes.data_as(C.POINTER(Hit)),
                                        C.c_void_p(stream) if stream else None))
        return out

    def trace_into(self, ray_ptr, n, hit_ptr, stream=None, timed=True):
        """rt_trace_rays on the caller's device memory (raw pointers to n rt_ray / n rt_hit, 16-byte aligned): device milliseconds, or
        None unless timed (then the call only enqueues one kernel)."""
        ms = C.c_float(0.0)
        _check(lib().rt_trace_rays(self._h, C.c_void_p(ray_ptr) if ray_ptr else None, int(n), C.c_void_p(hit_ptr) if hit_ptr else None,
                                   C.c_void_p(stream) if stream else None, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def occluded(self, origins, dirs, t_max=None, stream=None, timed=True, sort=False):
        """Is each ray blocked by some object at EPS < t < t_max (rt_occluded_rays; t_max: one value per ray, None = 1e6 for all)?
        Returns (torch int32 device tensor [n] of 1 / 0, device milliseconds or None).  sort=True: the same flags by way of rt_sort_rays
        (t_max gathered into the sorted order, the flags scattered back; the milliseconds then cover sort, query and scatter)."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        rays = self.rays(origins, dirs)
        if sort:
            with self._sorted(rays, stream) as q:
                tm = None if t_max is None else q.gathered(np.broadcast_to(np.asarray(t_max, dtype=np.float64), (q.n,)).copy(), 8)
                flags = q.result((q.n,), "int32")
                self.occluded_into(q.sorted_ptr, None if tm is None else tm.data_ptr(), q.n, flags.data_ptr(), stream=stream, timed=False)
                return q.scattered(flags, 4), (q.elapsed() if timed else None)
        d_rays = torch.from_numpy(rays.view(np.float64).reshape(-1, 6)).to(dev)
        d_tmax = None if t_max is None else torch.from_numpy(np.broadcast_to(np.asarray(t_max, dtype=np.float64), (len(rays),)).copy()).to(dev)
        out = torch.empty((len(rays),), dtype=torch.int32, device=dev)
        if stream:   # the uploads above ran on torch's current stream
            torch.cuda.current_stream().synchronize()
        ms = self.occluded_into(d_rays.data_ptr(), None if d_tmax is None else d_tmax.data_ptr(), len(rays), out.data_ptr(), stream=stream, timed=timed)
        return out, ms

    def occluded_into(self, ray_ptr, t_max_ptr, n, blocked_ptr, stream=None, timed=True):
        """rt_occluded_rays on the caller's device memory (raw pointers; t_max_ptr None = 1e6 for every ray)."""
        ms = C.c_float(0.0)
        _check(lib().rt_occluded_rays(self._h, C.c_void_p(ray_ptr) if ray_ptr else None, C.c_void_p(t_max_ptr) if t_max_ptr else None, int(n),
                                      C.c_void_p(blocked_ptr) if blocked_ptr else None, C.c_void_p(stream) if stream else None, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def shade(self, origins, dirs, stream=None, sort=False):
        """The reference's colour of every ray (rt_shade_rays_host; blocks): an [n, 4] float32 numpy array of (r, g, b, 1) -- what an
        RGBA32F pixel holds whose primary ray this is.  Directions are used as given.  Works in every context kind and format.
        sort=True: the same colours by way of rt_sort_rays, as trace() does it."""
        rays = self.rays(origins, dirs)
        if sort:
            with self._sorted(rays, stream) as q:
                rgba = q.result((q.n, 4), "float32")
                self.shade_into(q.sorted_ptr, q.n, rgba.data_ptr(), stream=stream, timed=False)
                return q.scattered(rgba, 16).cpu().numpy()
        out = np.zeros((len(rays), 4), dtype=np.float32)
        _check(lib().rt_shade_rays_host(self._h, rays.ctypes.data_as(C.POINTER(Ray)), len(rays), out.ctypes.data_as(C.POINTER(C.c_float)),
                                        C.c_void_p(stream) if stream else None))
        return out

    def shade_into(self, ray_ptr, n, rgba_ptr, hit_ptr=None, stream=None, timed=True):
        """rt_shade_rays on the caller's device memory (raw pointers to n rt_ray / n x 4 float32 / optionally n rt_hit, 16-byte
        aligned): device milliseconds, or None unless timed (then the call only enqueues one kernel)."""
        ms = C.c_float(0.0)
        _check(lib().rt_shade_rays(self._h, C.c_void_p(ray_ptr) if ray_ptr else None, int(n), C.c_void_p(rgba_ptr) if rgba_ptr else None,
                                   C.c_void_p(hit_ptr) if hit_ptr else None, C.c_void_p(stream) if stream else None, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def _max_segments(self, max_segments):
        return min(self._desc.max_reflections + 1, RT_PATH_MAX_SEGMENTS) if max_segments is None else int(max_segments)

    def paths(self, origins, dirs, max_segments=None, stream=None, sort=False):
        """The hits along every ray's mirror bounces (rt_trace_paths_host; blocks): (segments, last, ends) -- HIT_DTYPE records [M, n]
        of the segments (a segment the path did not reach is a miss record), HIT_DTYPE records [n] of the last hits, PATH_END_DTYPE
        records [n].  M = max_segments, by default max_reflections + 1 (every segment a path can have), at most 64; it limits what is
        stored, not how far a path is followed.  Works in every context kind.  sort=True: the same records by way of rt_sort_rays, as
        trace() does it (the segment planes scattered plane by plane)."""
        rays = self.rays(origins, dirs)
        m, n = self._max_segments(max_segments), len(rays)
        if sort:
            with self._sorted(rays, stream) as q:
                seg, last, ends = q.result((max(m, 1) * n, 6), "float64"), q.result((n, 6), "float64"), q.result((n, 4), "int32")
                self.paths_into(q.sorted_ptr, n, m, seg.data_ptr() if m else None, last.data_ptr(), ends.data_ptr(), stream=stream, timed=False)
                seg = q.scattered(seg, 48, planes=m).cpu().numpy().view(HIT_DTYPE).reshape(m, n) if m else np.zeros((0, n), dtype=HIT_DTYPE)
                return seg, q.scattered(last, 48).cpu().numpy().view(HIT_DTYPE).reshape(-1), q.scattered(ends, 16).cpu().numpy().view(PATH_END_DTYPE).reshape(-1)
        seg, last, ends = np.zeros((m, n), dtype=HIT_DTYPE), np.zeros(n, dtype=HIT_DTYPE), np.zeros(n, dtype=PATH_END_DTYPE)
        _check(lib().rt_trace_paths_host(self._h, rays.ctypes.data_as(C.POINTER(Ray)), n, m, seg.ctypes.data_as(C.POINTER(Hit)) if m else None,
                                         last.ctypes.data_as(C.POINTER(Hit)), ends.ctypes.data_as(C.POINTER(PathEnd)), C.c_void_p(stream) if stream else None))
        return seg, last, ends

    def paths_into(self, ray_ptr, n, max_segments, segments_ptr, last_ptr, ends_ptr, stream=None, timed=True):
        """rt_trace_paths on the caller's device memory (raw pointers to n rt_ray / max_segments x n rt_hit, None iff max_segments is 0 /
        optionally n rt_hit / n rt_path_end, 16-byte aligned): device milliseconds, or None unless timed (then the call only enqueues
        one kernel)."""
        ms = C.c_float(0.0)
        _check(lib().rt_trace_paths(self._h, C.c_void_p(ray_ptr) if ray_ptr else None, int(n), int(max_segments), C.c_void_p(segments_ptr) if segments_ptr else None,
                                    C.c_void_p(last_ptr) if last_ptr else None, C.c_void_p(ends_ptr) if ends_ptr else None, C.c_void_p(stream) if stream else None,
                                    C.byref(ms) if timed else None))
        return ms.value if timed else None

    @staticmethod
    def sort_work_bytes(n):
        """rt_sort_rays_work_bytes: the device work space rt_sort_rays needs for n rays."""
        return int(lib().rt_sort_rays_work_bytes(int(n)))

    def sort_rays_into(self, ray_ptr, n, sorted_ptr, perm_ptr, keys_ptr, work_ptr, work_bytes, stream=None, timed=True):
        """rt_sort_rays on the caller's device memory (raw pointers to n rt_ray / optionally n rt_ray / n uint32 / optionally n uint32 /
        work_bytes >= sort_work_bytes(n) of work space): device milliseconds, or None unless timed (then the call only enqueues kernels)."""
        ms = C.c_float(0.0)
        _check(lib().rt_sort_rays(self._h, C.c_void_p(ray_ptr) if ray_ptr else None, int(n), C.c_void_p(sorted_ptr) if sorted_ptr else None,
                                  C.c_void_p(perm_ptr) if perm_ptr else None, C.c_void_p(keys_ptr) if keys_ptr else None, C.c_void_p(work_ptr) if work_ptr else None,
                                  int(work_bytes), C.c_void_p(stream) if stream else None, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def permute_into(self, perm_ptr, n, src_ptr, dst_ptr, elem_bytes, planes=1, scatter=False, stream=None, timed=True):
        """rt_permute on the caller's device memory: planes x n records of elem_bytes, dst[i] = src[perm[i]], or with scatter
        dst[perm[i]] = src[i].  Device milliseconds, or None unless timed (then the call only enqueues one kernel)."""
        ms = C.c_float(0.0)
        _check(lib().rt_permute(self._h, C.c_void_p(perm_ptr) if perm_ptr else None, int(n), C.c_void_p(src_ptr) if src_ptr else None,
                                C.c_void_p(dst_ptr) if dst_ptr else None, int(elem_bytes), int(planes), 1 if scatter else 0, C.c_void_p(stream) if stream else None,
                                C.byref(ms) if timed else None))
        return ms.value if timed else None

    def sort_rays(self, origins, dirs, stream=None):
        """The rays in rt_sort_rays' order: (sorted RAY_DTYPE array, perm uint32 [n], keys uint32 [n]); sorted == rays[perm]."""
        with self._sorted(self.rays(origins, dirs), stream, keys=True) as q:
            q.sync()
            return (q.sorted.cpu().numpy().view(RAY_DTYPE).reshape(-1), q.perm.cpu().numpy().view(np.uint32), q.keys.cpu().numpy().view(np.uint32))

    def _sorted(self, rays, stream=None, keys=False):
        return _SortedRays(self, rays, stream, keys)

    def primary_rays(self, cam=None, rect=None, stream=None, timed=True):
        """The context's own primary rays of rect = (x0, y0, x1, y1) (inclusive, global coordinates, row 0 = bottom; None = the whole
        frame) as explicit rays (rt_primary_rays): a torch float64 device tensor [rows, columns, 6] of (origin, direction) -- bit for
        bit the rays the frame kernels trace -- and the device milliseconds (None unless timed)."""
        import torch
        x0, y0, x1, y1 = (0, 0, self.width - 1, self.height - 1) if rect is None else (int(v) for v in rect)
        out = torch.empty((max(y1 - y0 + 1, 0), max(x1 - x0 + 1, 0), 6), dtype=torch.float64, device=torch.device("cuda", torch.cuda.current_device()))
        ms = self.primary_rays_into(cam, rect, out.data_ptr() if out.numel() else None, stream=stream, timed=timed)
        return out, ms

    def primary_rays_into(self, cam, rect, ray_ptr, stream=None, timed=True):
        """rt_primary_rays into the caller's device memory (a raw pointer to one rt_ray per pixel of rect, 16-byte aligned)."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        keep, rp = self._rect(rect)
        ms = C.c_float(0.0)
        _check(lib().rt_primary_rays(self._h, _dptr(cam), rp, C.c_void_p(ray_ptr) if ray_ptr else None, C.c_void_p(stream) if stream else None,
                                     C.byref(ms) if timed else None))
        return ms.value if timed else None

    def pick_paths(self, xy, cam=None, max_segments=None, stream=None):
        """Pick through mirrors (rt_pick_paths; blocks): the paths of the primary rays of the pixels xy = [(x, y), ...] as (segments
        [M, n] HIT_DTYPE, ends [n] PATH_END_DTYPE).  Plane 0 is pick()'s record; ends["object"] is what the pixel finally shows where
        ends["end"] == RT_PATH_SURFACE."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        q = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
        m, n = self._max_segments(max_segments), q.shape[0]
        seg, ends = np.zeros((m, n), dtype=HIT_DTYPE), np.zeros(n, dtype=PATH_END_DTYPE)
        _check(lib().rt_pick_paths(self._h, _dptr(cam), q.ctypes.data_as(C.POINTER(C.c_uint32)), n, m, seg.ctypes.data_as(C.POINTER(Hit)) if m else None,
                                   ends.ctypes.data_as(C.POINTER(PathEnd)), C.c_void_p(stream) if stream else None))
        return seg, ends

    def set_scene(self, coefs=None, reflection=None, albedo=None, light_p=None, light_color=None, stream=None, reorder=False):
        """Replace the scene's raw descriptor arrays (numpy, rt_scene_desc layout; None = keep what the context holds) without a new
        context (rt_set_scene_host; blocks).  Raises SceneException when the update would change the scene's layout (include/mi355rt.h,
        "Scene updates"): nothing was written then.  reorder=True: reorder_scene() behind the applied update, on the same stream."""
        given = dict(coefs=coefs, reflection=reflection, albedo=albedo, light_p=light_p, light_color=light_color)
        keep = {n: np.ascontiguousarray(given[n], dtype=dt) for n, dt in SCENE_UPDATE_FIELDS if given[n] is not None}
        no, nl = self._desc.n_objects, self._desc.n_lights
        want = dict(coefs=no * RT_NCOEF, reflection=no, albedo=3 * no, light_p=3 * nl, light_color=3 * nl)
        for n, a in keep.items():
            if a.size != want[n]:
                raise ValueError(f"set_scene: {n} has {a.size} values, the scene takes {want[n]}")
        u = SceneUpdate(**{n: (a.ctypes.data if a.size else None) for n, a in keep.items()})
        _check(lib().rt_set_scene_host(self._h, C.byref(u), C.c_void_p(stream) if stream else None))
        if reorder:
            self.reorder_scene(stream)

    def set_scene_into(self, coefs=None, reflection=None, albedo=None, light_p=None, light_color=None, stream=None, reorder=False):
        """rt_set_scene on the caller's device memory (raw pointers, for example tensor.data_ptr(); None = keep): enqueues one kernel
        and returns -- capturable into a graph; whether it was applied is on the device (set_scene_status).  reorder=True: reorder_scene()
        is enqueued behind it on the same stream (a rejected update wrote nothing, and the reorder then re-sorts what the context held)."""
        u = SceneUpdate(coefs or None, reflection or None, albedo or None, light_p or None, light_color or None)
        _check(lib().rt_set_scene(self._h, C.byref(u), C.c_void_p(stream) if stream else None))
        if reorder:
            self.reorder_scene(stream)

    def reorder_scene(self, stream=None):
        """rt_reorder_scene: put the unit-sphere table the device holds into the spatial order a fresh Renderer on the current scene would
        choose and rebuild the chunk bounds -- kernels only, in the context's frame order, capturable into a graph.  No frame and no
        query changes, only the work they do: set_scene keeps the order chosen at creation, so the chunks of spheres that mix stop
        culling until this is called.  Enqueues nothing where stream_cull_reorder is False."""
        _check(lib().rt_reorder_scene(self._h, C.c_void_p(stream) if stream else None))

    @property
    def stream_cull_reorder(self):
        """True where reorder_scene() re-sorts: RT_FLAG_STREAM_CULL_REORDER on a context whose stream_cull is True
        (rt_get_stream_cull_reorder)."""
        n = C.c_uint32()
        _check(lib().rt_get_stream_cull_reorder(self._h, C.byref(n)))
        return bool(n.value)

    def set_scene_status(self):
        """Updates applied / rejected since the context was created and the reason / index of the last rejection (waits)."""
        a, r, why, idx = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        _check(lib().rt_set_scene_status(self._h, C.byref(a), C.byref(r), C.byref(why), C.byref(idx)))
        return dict(applied=int(a.value), rejected=int(r.value), reason=int(why.value), index=int(idx.value))

    def debug_scene_blob(self):
        """Diagnostics: the scene as the device holds it (blob, DevLight[], LightK[]) as bytes (rt_debug_scene_blob; waits)."""
        n = C.c_size_t()
        _check(lib().rt_debug_scene_blob(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        _check(lib().rt_debug_scene_blob(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(n)))
        return out

    @classmethod
    def _borrowed_view(cls, handle, desc, flags, fmt):
        """A Renderer over a context somebody else owns (MultiRenderer's query context): it never destroys it."""
        self = cls.__new__(cls)
        self._h, self._borrowed, self._desc = C.c_void_p(handle), True, desc
        self.width, self.height, self.fmt, self.flags = desc.width, desc.height, fmt, int(flags)
        n = C.c_uint32()
        _check(lib().rt_local_rows(self._h, C.byref(n)))
        self.local_rows = n.value
        _check(lib().rt_max_local_rows(self._h, C.byref(n)))
        self.max_local_rows = n.value
        self.pixel_bytes = lib().rt_pixel_bytes(self._h)
        return self

    def cleanup_update(self):
        if self._h and not getattr(self, "_borrowed", False):
            lib().rt_destroy(self._h)
        self._h = None

    close = cleanup_update

    def __del__(self):
        try:
            self.cleanup_update()
        except Exception:
            pass

    def row_map(self):
        rows = np.zeros(self.local_rows, dtype=np.uint32)
        if self.local_rows:
            _check(lib().rt_row_map(self._h, rows.ctypes.data_as(C.POINTER(C.c_uint32))))
        return rows

    def device_fb(self):
        return lib().rt_device_fb(self._h)

    def download(self):
        """Local rows of the output frame as numpy: float32 [rows, W, 4] (RGBA32F) or uint8 [rows, W, 4] (RGBA8); with supersampling
        the resolved pixels, not the samples."""
        dt = np.uint8 if self.fmt == RT_FMT_RGBA8 else np.float32
        out = np.empty((self.local_rows, self.width, 4), dtype=dt)
        if out.size:
            _check(lib().rt_download(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def assemble(self, gathered_ptr, full_ptr, stream=None):
        _check(lib().rt_assemble(self._h, C.c_void_p(gathered_ptr), C.c_void_p(full_ptr), C.c_void_p(stream) if stream else None))

    def assemble_planes(self, gathered_ptr, slot_stride_bytes, full_ptr, elem_bytes, stream=None):
        """rt_assemble_planes: assemble() for gathered planes of 4-, 8- or 16-byte elements (the G-buffer's), rank q's slot at
        gathered_ptr + q * slot_stride_bytes."""
        _check(lib().rt_assemble_planes(self._h, C.c_void_p(gathered_ptr) if gathered_ptr else None, int(slot_stride_bytes), C.c_void_p(full_ptr) if full_ptr else None,
                                        int(elem_bytes), C.c_void_p(stream) if stream else None))

    def merge_object_extents(self, parts_ptr, n_parts, out_ptr, stream=None):
        """rt_merge_object_extents: [n_parts][n_objects] records in device memory into n_objects records (sum / min / max)."""
        _check(lib().rt_merge_object_extents(self._h, C.c_void_p(parts_ptr) if parts_ptr else None, int(n_parts), C.c_void_p(out_ptr) if out_ptr else None,
                                             C.c_void_p(stream) if stream else None))

    # sparse transport of a frame (tiles with content only): see include/mi355rt.h
    @staticmethod
    def sparse_bytes(capacity_tiles):
        """Size of an RGBA8 message (rt_sparse_bytes)."""
        return int(lib().rt_sparse_bytes(int(capacity_tiles)))

    def sparse_msg_bytes(self, capacity_tiles):
        """Size of a message in this renderer's own format (rt_sparse_msg_bytes)."""
        return int(lib().rt_sparse_msg_bytes(int(self.fmt), int(capacity_tiles)))

    def update_sparse(self, msg_ptr, capacity_tiles, cam=None, stream=None, timed=True):
        """update() whose output is a sparse message (tiles with hits only) instead of a framebuffer."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        ms = C.c_float(0.0)
        _check(lib().rt_render_sparse(self._h, _dptr(cam), C.c_void_p(msg_ptr), int(capacity_tiles), C.c_void_p(stream) if stream else None,
                                      C.byref(ms) if timed else None))
        return ms.value if timed else None

    def pack_sparse(self, msg_ptr, capacity_tiles, fb_ptr=None, stream=None):
        _check(lib().rt_pack_sparse(self._h, C.c_void_p(fb_ptr) if fb_ptr else None, C.c_void_p(msg_ptr), int(capacity_tiles),
                                    C.c_void_p(stream) if stream else None))

    def assemble_sparse(self, gathered_ptr, capacity_tiles, full_ptr, stream=None):
        _check(lib().rt_assemble_sparse(self._h, C.c_void_p(gathered_ptr), int(capacity_tiles), C.c_void_p(full_ptr), C.c_void_p(stream) if stream else None))

    def sparse_stamp_bytes(self):
        return int(lib().rt_sparse_stamp_bytes(self._h))

    def assemble_sparse_incremental(self, gathered_ptr, capacity_tiles, full_ptr, stamps_ptr, frame_tag, stream=None):
        _check(lib().rt_assemble_sparse_incremental(self._h, C.c_void_p(gathered_ptr), int(capacity_tiles), C.c_void_p(full_ptr), C.c_void_p(stamps_ptr),
                                                    int(frame_tag), C.c_void_p(stream) if stream else None))

    def debug_counters(self):
        out = (C.c_uint64 * 32)()
        _check(lib().rt_debug_counters(self._h, out))
        return [int(v) for v in out]

    def stamp_rows(self):
        """Diagnostic builds: [n_rows, 16] uint64 per-wave rows of the last frame (see rt_debug_stamp_rows)."""
        n = C.c_size_t()
        _check(lib().rt_debug_stamp_rows(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 16), dtype=np.uint64)
        if n.value:
            _check(lib().rt_debug_stamp_rows(self._h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def wave_box(self, pts, use_masks):
        """Diagnostics (rt_debug_wave_box): the kernel's box helper alone.  pts = [n, 64, 3] float64, use_masks = [n] uint64 -> [n, 6] float32
        (lox, hix, loy, hiy, loz, hiz)."""
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        use_masks = np.ascontiguousarray(use_masks, dtype=np.uint64)
        assert pts.ndim == 3 and pts.shape[1:] == (64, 3) and use_masks.shape == (pts.shape[0],)
        out = np.zeros((pts.shape[0], 6), dtype=np.float32)
        _check(lib().rt_debug_wave_box(self._h, pts.ctypes.data_as(C.POINTER(C.c_double)), use_masks.ctypes.data_as(C.POINTER(C.c_uint64)), pts.shape[0],
                                       out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def counters(self):
        c = Counters()
        _check(lib().rt_get_counters(self._h, C.byref(c)))
        return c.as_dict()

    def counters_detail(self):
        """counters() plus the executed work split by surface class / culling kind / cubic solver branch (what bench.py's
        flop accounting multiplies with the per-unit costs of profiles/flop_table.json)."""
        d = self.counters()
        x = CountersDetail()
        _check(lib().rt_get_counters_detail(self._h, C.byref(x)))
        d["executed_by_class"] = dict(zip(("unitsq", "quadric", "linear", "cubic"), (int(v) for v in x.tests_executed)))
        d["solves_by_class"] = dict(zip(("unitsq", "quadric", "linear"), (int(v) for v in x.solves)))
        d["cull_by_kind"] = dict(zip(("tile", "primary", "shadow_directional", "shadow_point", "records"), (int(v) for v in x.cull_evals)))
        d["shadow_rays_traced"], d["hit_lights_shaded"], d["primary_rays_formed"] = int(x.shadow_rays_traced), int(x.hit_lights_shaded), int(x.primary_rays_formed)
        d["cubic_branches"] = dict(zip(("cardano", "trig", "quad", "linear"), (int(v) for v in x.cubic_branch)))
        d["cubic_points"] = int(x.cubic_points)
        d["cubic_refused"] = int(x.cubic_refused)
        return d


# The culling families of a context (csrc/rt_capi.cpp: CullFamily), one row each: the Renderer property that reads the decision and the
# Renderer method <property>_stats that reads the family's eight work words -- name, getter, debug reader, the two docstrings.
_CULL_FAMILIES = (
    ("stream_cull", "rt_get_stream_cull", "rt_debug_stream_cull",
     """True where update() culls whole chunks of the unit-sphere table: RT_FLAG_STREAM_CULL on a streamed context whose culling is on.""",
     """The culling kernel's eight work words since the context was created (rt_debug_stream_cull; waits).  They exist only where
        stream_cull is True and MI355RT_STREAM_CULL_STATS=1 was in the environment when the context was created."""),
    ("stream_cull_adaptive", "rt_get_stream_cull_adaptive", "rt_debug_stream_cull_adaptive",
     """True where the halo and refine passes of an adaptive frame cull whole chunks of the unit-sphere table as well: stream_cull and
        streamed_adaptive on a scene of at least two chunks (rt_get_stream_cull_adaptive).""",
     """The eight work words of the culling halo and refine kernels since the context was created (rt_debug_stream_cull_adaptive;
        waits).  They exist only where stream_cull_adaptive is True, MI355RT_STREAM_CULL_STATS=1 was in the environment when the context
        was created, and the scene does not hold both general quadrics and degree-3 objects."""),
    ("stream_cull_bounce", "rt_get_stream_cull_bounce", "rt_debug_stream_cull_bounce",
     """True where update() culls the unit-sphere chunks of its bounce rays per ray as well: RT_FLAG_STREAM_CULL_BOUNCE on a context whose
        stream_cull is True, with a mirror in the scene, max_reflections >= 1 and at least two chunks (rt_get_stream_cull_bounce).""",
     """The eight work words of the bounce queries since the context was created (rt_debug_stream_cull_bounce; waits).  They exist only
        where stream_cull_bounce is True and MI355RT_STREAM_CULL_STATS=1 was in the environment when the context was created."""),
    ("stream_cull_rays", "rt_get_stream_cull_rays", "rt_debug_stream_cull_rays",
     """True where the ray queries (trace_rays, occluded_rays, shade_rays, trace_paths, pick_paths) cull the unit-sphere chunks per
        caller-supplied ray: RT_FLAG_STREAM_CULL_RAYS on a context whose stream_cull and streamed_queries are True, with at least two
        chunks (rt_get_stream_cull_rays).""",
     """The eight work words the culled ray queries share, since the context was created (rt_debug_stream_cull_rays; waits).  They exist
        only where stream_cull_rays is True and MI355RT_STREAM_CULL_STATS=1 was in the environment when the context was created."""),
    ("stream_cull_pixels", "rt_get_stream_cull_pixels", "rt_debug_stream_cull_pixels",
     """True where the pixel queries (gbuffer, pick, object_extents) cull the unit-sphere chunks by the block's cone:
        RT_FLAG_STREAM_CULL_PIXELS on a context whose stream_cull and streamed_queries are True, with at least two chunks
        (rt_get_stream_cull_pixels).""",
     """The eight work words the culled pixel queries share, since the context was created (rt_debug_stream_cull_pixels; waits).  They
        exist only where stream_cull_pixels is True and MI355RT_STREAM_CULL_STATS=1 was in the environment when the context was created."""),
)


def _cull_family_members(name, getter, debug, flag_doc, stats_doc):
    def flag(self):
        n = C.c_uint32()
        _check(getattr(lib(), getter)(self._h, C.byref(n)))
        return bool(n.value)

    def stats(self):
        w = (C.c_uint64 * 8)()
        _check(getattr(lib(), debug)(self._h, w))
        return [int(v) for v in w]

    flag.__name__, stats.__name__ = name, name + "_stats"
    flag.__qualname__, stats.__qualname__ = "Renderer." + name, "Renderer." + name + "_stats"
    flag.__doc__, stats.__doc__ = flag_doc, stats_doc
    setattr(Renderer, name, property(flag))
    setattr(Renderer, name + "_stats", stats)


for _row in _CULL_FAMILIES:
    _cull_family_members(*_row)


class MultiRenderer:
    """init_update / update / cleanup_update over several GPUs of one node (rt_create_multi ...): the frame ends up on devices[0]."""

    def __init__(self, scene, devices, band_rows=16, parts=1, flags=RT_FLAG_STRICT, fmt=RT_FMT_RGBA32F, ssaa_min_cos=None):
        self._h = None
        d = scene.desc() if isinstance(scene, Scene) else scene
        self._desc = d
        self._devices, self._flags, self._query = [int(v) for v in devices], int(flags) & 0xFFFF, None
        devs = (C.c_int * len(devices))(*[int(v) for v in devices])
        h = C.c_void_p()
        _check(multi_lib().rt_create_multi(C.byref(h), C.byref(d), devs, len(devices), int(band_rows), int(parts), int(flags), int(fmt)))
        self._h = h
        self.width, self.height, self.fmt = d.width, d.height, fmt
        n, t = C.c_uint32(), C.c_uint32()
        _check(multi_lib().rt_multi_info(self._h, C.byref(n), C.byref(t)))
        self.n_contexts, self.transport = n.value, {0: "in place", 1: "device copies", 2: "rccl"}[t.value]
        if ssaa_min_cos is not None:
            self.set_ssaa_geometry(ssaa_min_cos)

    def last_transfer(self):
        """(bytes_sent, bytes_dense) of the last frame: what travelled to the root, and what the dense transport moves."""
        sent, dense = C.c_uint64(), C.c_uint64()
        _check(multi_lib().rt_multi_last_transfer(self._h, C.byref(sent), C.byref(dense)))
        return int(sent.value), int(dense.value)

    def set_ssaa_threshold(self, tau):
        """Renderer.set_ssaa_threshold on every context (RT_FLAG_SSAA_ADAPTIVE objects only)."""
        _check(multi_lib().rt_multi_set_ssaa_threshold(self._h, float(tau)))

    def set_ssaa_geometry(self, min_cos):
        """Renderer.set_ssaa_geometry on every context (RT_FLAG_SSAA_GEOMETRY objects only)."""
        _check(multi_lib().rt_multi_set_ssaa_geometry(self._h, float(min_cos)))

    def update(self, cam=None, full_ptr=None, timed=True):
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        ms = C.c_float(0.0)
        _check(multi_lib().rt_render_multi(self._h, _dptr(cam), C.c_void_p(full_ptr) if full_ptr else None, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def wait(self):
        _check(multi_lib().rt_multi_wait(self._h))

    @property
    def stream(self):
        """rt_multi_stream: the root's stream frames, planes and extents are complete on, and the one the queries run on."""
        return multi_lib().rt_multi_stream(self._h)

    def set_scene(self, coefs=None, reflection=None, albedo=None, light_p=None, light_color=None):
        """Renderer.set_scene on every context (rt_set_scene_multi): enqueues only, in every context's frame order; whether the update
        was applied is on the devices (set_scene_status)."""
        given = dict(coefs=coefs, reflection=reflection, albedo=albedo, light_p=light_p, light_color=light_color)
        keep = {n: np.ascontiguousarray(given[n], dtype=dt) for n, dt in SCENE_UPDATE_FIELDS if given[n] is not None}
        no, nl = self._desc.n_objects, self._desc.n_lights
        want = dict(coefs=no * RT_NCOEF, reflection=no, albedo=3 * no, light_p=3 * nl, light_color=3 * nl)
        for n, a in keep.items():
            if a.size != want[n]:
                raise ValueError(f"set_scene: {n} has {a.size} values, the scene takes {want[n]}")
        u = SceneUpdate(**{n: (a.ctypes.data if a.size else None) for n, a in keep.items()})
        _check(multi_lib().rt_set_scene_multi(self._h, C.byref(u)))

    def reorder_scene(self):
        """Renderer.reorder_scene on every context (rt_reorder_scene_multi): enqueues only, in every context's frame order."""
        _check(multi_lib().rt_reorder_scene_multi(self._h))

    def set_scene_status(self):
        """Updates applied / rejected and the reason / index of the last rejection, the same on every context (waits for all of them)."""
        a, r, why, idx = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        _check(multi_lib().rt_multi_set_scene_status(self._h, C.byref(a), C.byref(r), C.byref(why), C.byref(idx)))
        return dict(applied=int(a.value), rejected=int(r.value), reason=int(why.value), index=int(idx.value))

    def gbuffer(self, cam=None, object=True, t=True, normal=True, timed=True):
        """The primary-hit G-buffer of the whole frame on devices[0] (rt_render_gbuffer_multi): torch device tensors (object int32
        [H, W], t float64 [H, W], normal float32 [H, W, 4]; None for a plane not asked for) and the device milliseconds (None unless
        timed; then complete on `stream`, not on the host)."""
        import torch
        dev = torch.device("cuda", self._devices[0])
        h, w = self.height, self.width
        po = torch.empty((h, w), dtype=torch.int32, device=dev) if object else None
        pt = torch.empty((h, w), dtype=torch.float64, device=dev) if t else None
        pn = torch.empty((h, w, 4), dtype=torch.float32, device=dev) if normal else None
        torch.cuda.synchronize(dev)   # (the allocations are torch's; the planes are written on the object's own stream)
        ms = self.gbuffer_into(cam, po.data_ptr() if object else None, pt.data_ptr() if t else None, pn.data_ptr() if normal else None, timed=timed)
        return po, pt, pn, ms

    def gbuffer_into(self, cam, object_ptr, t_ptr, normal_ptr, timed=True):
        """rt_render_gbuffer_multi into the caller's device memory on devices[0] (raw pointers, None = plane not written)."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        ms = C.c_float(0.0)
        _check(multi_lib().rt_render_gbuffer_multi(self._h, _dptr(cam), C.c_void_p(object_ptr) if object_ptr else None, C.c_void_p(t_ptr) if t_ptr else None,
                                                   C.c_void_p(normal_ptr) if normal_ptr else None, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def object_extents(self, cam=None, rect=None):
        """Renderer.object_extents of the whole frame: the contexts' records merged on the root (rt_object_extents_multi_host; blocks)."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        keep, rp = Renderer._rect(rect)
        out = np.zeros(self._desc.n_objects, dtype=EXTENT_DTYPE)
        buf = out if len(out) else np.zeros(1, dtype=EXTENT_DTYPE)
        _check(multi_lib().rt_object_extents_multi_host(self._h, _dptr(cam), rp, buf.ctypes.data_as(C.c_void_p)))
        return out

    def object_extents_into(self, cam, rect, out_ptr, timed=True):
        """rt_object_extents_multi into the caller's device memory on devices[0] (n_objects records of 40 bytes, 8-byte aligned)."""
        cam = np.ascontiguousarray(IDENTITY if cam is None else cam, dtype=np.float64).reshape(16)
        keep, rp = Renderer._rect(rect)
        ms = C.c_float(0.0)
        _check(multi_lib().rt_object_extents_multi(self._h, _dptr(cam), rp, C.c_void_p(out_ptr) if out_ptr else None, C.byref(ms) if timed else None))
        return ms.value if timed else None

    @property
    def stream_cull_bounce(self):
        """Renderer.stream_cull_bounce of the contexts: they share scene, flags and max_reflections, hence the decision (read from
        rt_multi_query_ctx's context)."""
        return self.query.stream_cull_bounce

    @property
    def stream_groups(self):
        """Renderer.stream_groups of the contexts: they share scene and flags, hence the decision (read from rt_multi_query_ctx's context)."""
        return self.query.stream_groups

    @property
    def stream_cull_rays(self):
        """Renderer.stream_cull_rays of rt_multi_query_ctx's context: the one that answers the ray queries."""
        return self.query.stream_cull_rays

    @property
    def stream_cull_pixels(self):
        """Renderer.stream_cull_pixels of rt_multi_query_ctx's context (the contexts share scene and flags, hence the decision)."""
        return self.query.stream_cull_pixels

    @property
    def query(self):
        """A Renderer view of rt_multi_query_ctx's context, for the queries that depend neither on rows nor on frame state.  Borrowed:
        it lives as long as this object and never destroys the context.  Use it on `stream` (the methods below do)."""
        if self._query is None:
            self._query = Renderer._borrowed_view(multi_lib().rt_multi_query_ctx(self._h), self._desc, self._flags, self.fmt)
        return self._query

    def pick(self, xy, cam=None):
        return self.query.pick(xy, cam=cam, stream=self.stream)

    def pick_paths(self, xy, cam=None, max_segments=None):
        return self.query.pick_paths(xy, cam=cam, max_segments=max_segments, stream=self.stream)

    def trace(self, origins, dirs):
        return self.query.trace(origins, dirs, stream=self.stream)

    def occluded(self, origins, dirs, t_max=None, timed=True):
        return self.query.occluded(origins, dirs, t_max=t_max, stream=self.stream, timed=timed)

    def shade(self, origins, dirs):
        return self.query.shade(origins, dirs, stream=self.stream)

    def paths(self, origins, dirs, max_segments=None):
        return self.query.paths(origins, dirs, max_segments=max_segments, stream=self.stream)

    def download(self):
        dt = np.uint8 if self.fmt == RT_FMT_RGBA8 else np.float32
        out = np.empty((self.height, self.width, 4), dtype=dt)
        _check(multi_lib().rt_multi_download(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def cleanup_update(self):
        if self._h:
            if self._query is not None:   # (the view dies with the object it borrows from)
                self._query.cleanup_update()
            multi_lib().rt_multi_destroy(self._h)
            self._h = None

    close = cleanup_update

    def __del__(self):
        try:
            self.cleanup_update()
        except Exception:
            pass


# The base library alone does not make a build: a caller that checks for it (tests/conftest.py) must not meet a build that another
# process is still running, or one that lost a product since (the host driver lives under tests/).  Complete such a build, under
# the build lock, before anything uses it; a complete build costs a few stat calls here.
if os.path.exists(BUILD_PRODUCTS[0]) and not all(os.path.exists(p) for p in BUILD_PRODUCTS[1:]):
    build()
