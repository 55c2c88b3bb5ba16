"""Python host binding of the HIP library (lib/libdpe_mvs.so) through its C-ABI.

There is no CPU fallback: if the library is missing this module raises at import.  The library
is built in-tree by `make -C dpe-mvs_amd` (or `__graft_entry__.build()`).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPE_MVS_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libdpe_mvs.so")

EXPORTED = [
    "dpe_params_default", "dpe_create", "dpe_destroy", "dpe_last_error", "dpe_pm_stage",
    "dpe_pm_execute", "dpe_pm_fetch", "dpe_pm_run", "dpe_pm_device_planes", "dpe_pm_export_depth",
    "dpe_pm_last_timings", "dpe_set_timing", "dpe_set_counting", "dpe_pm_last_counts",
    "dpe_fusion_stage", "dpe_fusion_candidates",
    "dpe_fusion_tat_begin", "dpe_fusion_tat_image", "dpe_fusion_tat_wait", "dpe_fusion_tat_mask",
    "dpe_pm_stage_resident", "dpe_state_save", "dpe_state_snapshot", "dpe_state_fetch", "dpe_state_export_depth",
    "dpe_state_import_depth", "dpe_state_clear", "dpe_device_buffer", "dpe_device_copy",
    "dpe_resize_linear", "dpe_resize_u8", "dpe_canny", "dpe_roberts_threshold",
    "dpe_state_render", "dpe_state_render_jpeg_blocks", "dpe_state_render_wait", "dpe_viz_render_arrays",
    "dpe_jpeg_blocks_device", "dpe_viz_launches", "dpe_live_device_bytes",
    "dpe_state_point_cloud", "dpe_state_point_cloud_wait", "dpe_point_cloud_arrays", "dpe_points_launches",
    "dpe_fusion_consistency", "dpe_consistency_launches",
    "dpe_cloud_nn", "dpe_cloud_nn_pair", "dpe_cloud_launches", "dpe_cloud_last_timings", "dpe_cloud_voxel",
    "dpe_cloud_nn_index", "dpe_cloud_icp_stage", "dpe_cloud_icp_step",
    "dpe_cloud_render_stage", "dpe_cloud_render_view", "dpe_depth_score",
    "dpe_cloud_normals", "dpe_cloud_render_stage_normals", "dpe_cloud_render_view_normals", "dpe_normal_score",
]

VIZ_DEPTH, VIZ_NORMAL, VIZ_WEAK = 0, 1, 2
POINTS_ALL, POINTS_STRONG = 1, 2

CLASSES = ["setup", "init", "strong", "ransac", "weak", "filter", "depth_to_weak", "local_refine"]


def load_library(path: str = LIB_PATH) -> C.CDLL:
    if not os.path.exists(path):
        raise RuntimeError(f"HIP library not built: {path} (run `make -C dpe-mvs_amd`)")
    lib = C.CDLL(path)
    lib.dpe_params_default.argtypes = [C.POINTER(_abi.DpePatchMatchParams)]
    lib.dpe_params_default.restype = None
    lib.dpe_create.argtypes = [C.c_int]
    lib.dpe_create.restype = C.c_void_p
    lib.dpe_destroy.argtypes = [C.c_void_p]
    lib.dpe_destroy.restype = None
    lib.dpe_last_error.argtypes = []
    lib.dpe_last_error.restype = C.c_char_p
    for fn in ("dpe_pm_stage", "dpe_pm_run"):
        getattr(lib, fn).argtypes = [C.c_void_p, C.POINTER(_abi.DpePassInput), C.POINTER(_abi.DpePassState)]
        getattr(lib, fn).restype = C.c_int
    lib.dpe_pm_execute.argtypes = [C.c_void_p, C.c_void_p]
    lib.dpe_pm_execute.restype = C.c_int
    lib.dpe_pm_fetch.argtypes = [C.c_void_p, C.POINTER(_abi.DpePassState)]
    lib.dpe_pm_fetch.restype = C.c_int
    lib.dpe_pm_device_planes.argtypes = [C.c_void_p]
    lib.dpe_pm_device_planes.restype = C.c_void_p
    lib.dpe_pm_export_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dpe_pm_export_depth.restype = C.c_int
    lib.dpe_pm_last_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    lib.dpe_pm_last_timings.restype = C.c_int
    lib.dpe_set_timing.argtypes = [C.c_void_p, C.c_int]
    lib.dpe_set_timing.restype = None
    lib.dpe_set_counting.argtypes = [C.c_void_p, C.c_int]
    lib.dpe_set_counting.restype = None
    lib.dpe_pm_last_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
    lib.dpe_pm_last_counts.restype = C.c_int
    lib.dpe_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.dpe_set_option.restype = C.c_int
    lib.dpe_pm_last_stat.argtypes = [C.c_void_p, C.c_int]
    lib.dpe_pm_last_stat.restype = C.c_longlong
    lib.dpe_fusion_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.dpe_fusion_stage.restype = C.c_int
    lib.dpe_fusion_candidates.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.dpe_fusion_candidates.restype = C.c_int
    lib.dpe_fusion_consistency.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    lib.dpe_fusion_consistency.restype = C.c_int
    lib.dpe_consistency_launches.argtypes = []
    lib.dpe_consistency_launches.restype = C.c_longlong
    lib.dpe_fusion_tat_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dpe_fusion_tat_begin.restype = C.c_int
    lib.dpe_fusion_tat_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dpe_fusion_tat_image.restype = C.c_int
    lib.dpe_fusion_tat_wait.argtypes = [C.c_void_p]
    lib.dpe_fusion_tat_wait.restype = C.c_int
    lib.dpe_fusion_tat_mask.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.dpe_fusion_tat_mask.restype = C.c_int
    lib.dpe_resize_linear.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.dpe_resize_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.dpe_canny.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]
    lib.dpe_roberts_threshold.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    for fn in ("dpe_resize_linear", "dpe_resize_u8", "dpe_canny", "dpe_roberts_threshold"):
        getattr(lib, fn).restype = C.c_int
    lib.dpe_state_save.argtypes = [C.c_void_p, C.c_int]
    lib.dpe_state_save.restype = C.c_int
    lib.dpe_state_fetch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    lib.dpe_state_fetch.restype = C.c_int
    lib.dpe_device_buffer.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    lib.dpe_device_buffer.restype = C.c_void_p
    lib.dpe_device_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.dpe_device_copy.restype = C.c_int
    lib.dpe_state_import_depth.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.dpe_state_import_depth.restype = C.c_int
    lib.dpe_sync.argtypes = [C.c_void_p]
    lib.dpe_sync.restype = C.c_int
    lib.dpe_state_render.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]
    lib.dpe_state_render.restype = C.c_int
    lib.dpe_state_render_jpeg_blocks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p,
                                                 C.c_size_t, C.c_void_p]
    lib.dpe_state_render_jpeg_blocks.restype = C.c_int
    lib.dpe_state_render_wait.argtypes = [C.c_void_p, C.c_void_p]
    lib.dpe_state_render_wait.restype = C.c_int
    lib.dpe_viz_render_arrays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_float, C.c_float, C.c_void_p]
    lib.dpe_viz_render_arrays.restype = C.c_int
    lib.dpe_jpeg_blocks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.dpe_jpeg_blocks_device.restype = C.c_int
    lib.dpe_viz_launches.argtypes = []
    lib.dpe_viz_launches.restype = C.c_longlong
    lib.dpe_state_point_cloud.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(_abi.DpeCamera), C.c_void_p, C.c_float,
                                          C.c_float, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    lib.dpe_state_point_cloud.restype = C.c_int
    lib.dpe_state_point_cloud_wait.argtypes = [C.c_void_p, C.c_void_p]
    lib.dpe_state_point_cloud_wait.restype = C.c_int
    lib.dpe_point_cloud_arrays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.POINTER(_abi.DpeCamera), C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_size_t)]
    lib.dpe_point_cloud_arrays.restype = C.c_int
    lib.dpe_points_launches.argtypes = []
    lib.dpe_points_launches.restype = C.c_longlong
    lib.dpe_cloud_nn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
    lib.dpe_cloud_nn.restype = C.c_int
    lib.dpe_cloud_nn_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]
    lib.dpe_cloud_nn_pair.restype = C.c_int
    lib.dpe_cloud_launches.argtypes = []
    lib.dpe_cloud_launches.restype = C.c_longlong
    lib.dpe_cloud_last_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    lib.dpe_cloud_last_timings.restype = C.c_int
    lib.dpe_cloud_voxel.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dpe_cloud_voxel.restype = C.c_int
    lib.dpe_cloud_nn_index.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]
    lib.dpe_cloud_nn_index.restype = C.c_int
    lib.dpe_cloud_icp_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float]
    lib.dpe_cloud_icp_stage.restype = C.c_int
    lib.dpe_cloud_icp_step.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DpeIcpSums)]
    lib.dpe_cloud_icp_step.restype = C.c_int
    lib.dpe_cloud_render_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.dpe_cloud_render_stage.restype = C.c_int
    lib.dpe_cloud_render_view.argtypes = [C.c_void_p, C.POINTER(_abi.DpeCamera), C.c_int, C.c_void_p]
    lib.dpe_cloud_render_view.restype = C.c_int
    lib.dpe_depth_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                    C.POINTER(_abi.DpeDepthScore), C.c_void_p]
    lib.dpe_depth_score.restype = C.c_int
    lib.dpe_cloud_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dpe_cloud_normals.restype = C.c_int
    lib.dpe_cloud_render_stage_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.dpe_cloud_render_stage_normals.restype = C.c_int
    lib.dpe_cloud_render_view_normals.argtypes = [C.c_void_p, C.POINTER(_abi.DpeCamera), C.c_int, C.c_void_p, C.c_void_p]
    lib.dpe_cloud_render_view_normals.restype = C.c_int
    lib.dpe_normal_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                     C.POINTER(_abi.DpeNormalScore), C.c_void_p]
    lib.dpe_normal_score.restype = C.c_int
    for fn in ("dpe_state_clear", "dpe_image_cache_clear"):
        getattr(lib, fn).argtypes = [C.c_void_p]
        getattr(lib, fn).restype = None
    lib.dpe_live_device_bytes.argtypes = []
    lib.dpe_live_device_bytes.restype = C.c_longlong
    return lib


DpeIcpSums = _abi.DpeIcpSums


def fusion_view_array(views):
    """[(depth f32 [H,W], normal f32 [H,W,3], DpeCamera)] -> (DpeFusionView array, arrays to keep alive)."""
    arr = (_abi.DpeFusionView * len(views))()
    keep = []
    for k, (d, n, cam) in enumerate(views):
        d = np.ascontiguousarray(d, np.float32)
        n = np.ascontiguousarray(n, np.float32)
        keep += [d, n]
        arr[k] = _abi.DpeFusionView(d.shape[1], d.shape[0], cam, d.ctypes.data, n.ctypes.data)
    return arr, keep


def as_cloud(points) -> np.ndarray:
    """A cloud as the C-ABI takes it: contiguous f32 [k, 3] (its memory is valid for k = 0 too)."""
    a = np.ascontiguousarray(points, np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        if a.size:
            raise ValueError("expected points of shape [k, 3]")
        a = np.empty((0, 3), np.float32)
    return a


_LIB = load_library()


class DpeError(RuntimeError):
    pass


def _check(rc: int, what: str):
    if rc != 0:
        msg = _LIB.dpe_last_error().decode(errors="replace")
        raise DpeError(f"{what} failed ({rc}): {msg}")


class PatchMatchContext:
    """One HIP device context (the reference's per-image `DPE` object minus the file I/O)."""

    def __init__(self, device: int = 0):
        self._ctx = _LIB.dpe_create(int(device))
        if not self._ctx:
            raise DpeError("dpe_create failed: " + _LIB.dpe_last_error().decode(errors="replace"))
        self._bufs = None

    def close(self):
        if self._ctx:
            _LIB.dpe_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # EdgeSegment's data-parallel stages (include/dpe_mvs.h; bit-identical to host/edges.cpp)
    def resize_linear(self, img: np.ndarray, nw: int, nh: int) -> np.ndarray:
        src = np.ascontiguousarray(img, np.float32)
        out = np.empty((nh, nw), np.float32)
        _check(_LIB.dpe_resize_linear(self._ctx, src.ctypes.data, src.shape[1], src.shape[0], out.ctypes.data, nw, nh),
               "dpe_resize_linear")
        return out

    def resize_u8(self, img: np.ndarray, nw: int, nh: int) -> np.ndarray:
        src = np.ascontiguousarray(img, np.uint8)
        out = np.empty((nh, nw), np.uint8)
        _check(_LIB.dpe_resize_u8(self._ctx, src.ctypes.data, src.shape[1], src.shape[0], out.ctypes.data, nw, nh),
               "dpe_resize_u8")
        return out

    def canny(self, img: np.ndarray, low: float, high: float) -> np.ndarray:
        src = np.ascontiguousarray(img, np.uint8)
        out = np.empty_like(src)
        _check(_LIB.dpe_canny(self._ctx, src.ctypes.data, src.shape[1], src.shape[0], float(low), float(high),
                              out.ctypes.data), "dpe_canny")
        return out

    def roberts_threshold(self, img: np.ndarray, thr: int) -> np.ndarray:
        src = np.ascontiguousarray(img, np.uint8)
        out = np.empty_like(src)
        _check(_LIB.dpe_roberts_threshold(self._ctx, src.ctypes.data, src.shape[1], src.shape[0], int(thr), out.ctypes.data),
               "dpe_roberts_threshold")
        return out

    def set_timing(self, on: bool):
        _LIB.dpe_set_timing(self._ctx, 1 if on else 0)

    def stage(self, pass_input: dict, state: dict):
        self._bufs = _abi.PassBuffers(pass_input, state)
        _check(_LIB.dpe_pm_stage(self._ctx, C.byref(self._bufs.inp), C.byref(self._bufs.st)), "dpe_pm_stage")

    def execute(self, stream: int | None = None):
        _check(_LIB.dpe_pm_execute(self._ctx, C.c_void_p(stream or 0)), "dpe_pm_execute")

    def fetch(self) -> dict:
        _check(_LIB.dpe_pm_fetch(self._ctx, C.byref(self._bufs.st)), "dpe_pm_fetch")
        return {k: v.copy() for k, v in self._bufs.outputs().items()}

    def run(self, pass_input: dict, state: dict) -> dict:
        self.stage(pass_input, state)
        self.execute()
        return self.fetch()

    def set_counting(self, on: bool):
        _LIB.dpe_set_counting(self._ctx, 1 if on else 0)

    def set_option(self, option: int, value: int):
        _check(_LIB.dpe_set_option(self._ctx, int(option), int(value)), "dpe_set_option")

    def last_stat(self, stat: int) -> int:
        return int(_LIB.dpe_pm_last_stat(self._ctx, int(stat)))

    def timings(self) -> dict:
        """{'total': ms, <class>: summed kernel ms} of the last execute (timing enabled)."""
        buf = (C.c_float * 9)()
        n = _LIB.dpe_pm_last_timings(self._ctx, buf, 9)
        out = {"total": float(buf[0])}
        for i, name in enumerate(CLASSES):
            if 1 + i < n:
                out[name] = float(buf[1 + i])
        return out

    def counts(self) -> dict:
        """{<class>: {'ncc', 'taps', 'geom', 'launches'}} of the last execute (counting enabled)."""
        buf = (C.c_ulonglong * 32)()
        _LIB.dpe_pm_last_counts(self._ctx, buf, 32)
        return {name: {"ncc": int(buf[4 * i]), "taps": int(buf[4 * i + 1]), "geom": int(buf[4 * i + 2]),
                       "launches": int(buf[4 * i + 3])} for i, name in enumerate(CLASSES)}

    def fusion_stage(self, views):
        """Uploads views = [(depth f32 [H, W], normal f32 [H, W, 3], DpeCamera)] (dpe_fusion_stage); they stay
        resident for fusion_consistency."""
        arr, keep = fusion_view_array(views)
        _check(_LIB.dpe_fusion_stage(self._ctx, arr, len(views)), "dpe_fusion_stage")
        self._staged_sizes = [(v.width, v.height) for v in arr]

    def fusion_consistency(self, ref: int, src, dot_threshold: float, min_views: int, want_count: bool = True,
                           want_depth: bool = True) -> tuple:
        """The consistency maps of staged view `ref` against the staged views `src` on the GPU
        (dpe_fusion_consistency): (count u8 [H, W], depth_filtered f32 [H, W]); an output that is not
        wanted is passed as NULL and returned as None.  `dot_threshold`: pipeline.consistency_dot_threshold()."""
        sizes = getattr(self, "_staged_sizes", [])
        w, h = sizes[ref] if 0 <= ref < len(sizes) else (1, 1)
        s = np.ascontiguousarray(src, np.int32)
        count = np.empty((h, w), np.uint8) if want_count else None
        depth = np.empty((h, w), np.float32) if want_depth else None
        _check(_LIB.dpe_fusion_consistency(self._ctx, int(ref), s.ctypes.data if len(s) else None, len(s), float(dot_threshold),
                                           int(min_views), None if count is None else count.ctypes.data,
                                           None if depth is None else depth.ctypes.data), "dpe_fusion_consistency")
        return count, depth

    def fusion_candidates(self, views, ref: int, src) -> tuple:
        """RunFusion's projection tests on the GPU (dpe_fusion_stage + dpe_fusion_candidates) for
        views = [(depth, normal, DpeCamera)]: (idx int32 [L*ns], val f32 [L*ns*3])."""
        arr, keep = fusion_view_array(views)
        _check(_LIB.dpe_fusion_stage(self._ctx, arr, len(views)), "dpe_fusion_stage")
        s = np.ascontiguousarray(src, np.int32)
        L = views[ref][0].size
        idx, val = np.empty(L * len(s), np.int32), np.empty(L * len(s) * 3, np.float32)
        _check(_LIB.dpe_fusion_candidates(self._ctx, int(ref), s.ctypes.data, len(s), idx.ctypes.data, val.ctypes.data),
               "dpe_fusion_candidates")
        return idx, val

    # HBM-resident state and the viz medium results rendered from it (include/dpe_mvs.h)
    def state_save(self, image_id: int):
        _check(_LIB.dpe_state_save(self._ctx, int(image_id)), "dpe_state_save")

    def state_clear(self):
        _LIB.dpe_state_clear(self._ctx)

    def image_cache_clear(self):
        _LIB.dpe_image_cache_clear(self._ctx)

    def state_fetch(self, image_id: int) -> dict:
        """{'depth' f32 [H,W], 'normal' f32 [H,W,3], 'weak' u8 [H,W], 'sel' u32 [H,W]} of a saved state."""
        w, h = C.c_int(), C.c_int()
        _check(_LIB.dpe_state_fetch(self._ctx, int(image_id), C.byref(w), C.byref(h), None, None, None, None), "dpe_state_fetch")
        H, W = h.value, w.value
        out = {"depth": np.empty((H, W), np.float32), "normal": np.empty((H, W, 3), np.float32),
               "weak": np.empty((H, W), np.uint8), "sel": np.empty((H, W), np.uint32)}
        _check(_LIB.dpe_state_fetch(self._ctx, int(image_id), C.byref(w), C.byref(h), out["depth"].ctypes.data,
                                    out["normal"].ctypes.data, out["weak"].ctypes.data, out["sel"].ctypes.data), "dpe_state_fetch")
        return out

    def state_import_depth(self, image_id: int, depth: np.ndarray):
        """A depth-only state (what another rank's image is after an exchange) from a host f32 [H, W] map."""
        d = np.ascontiguousarray(depth, np.float32)
        dev = _LIB.dpe_device_buffer(self._ctx, 0, d.size)
        if not dev:
            raise DpeError("dpe_device_buffer failed: " + _LIB.dpe_last_error().decode(errors="replace"))
        _check(_LIB.dpe_device_copy(self._ctx, dev, d.ctypes.data, d.nbytes, 0), "dpe_device_copy")
        _check(_LIB.dpe_state_import_depth(self._ctx, int(image_id), d.shape[1], d.shape[0], dev, None), "dpe_state_import_depth")
        _check(_LIB.dpe_sync(self._ctx), "dpe_sync")

    def _state_size(self, image_id: int):
        w, h = C.c_int(), C.c_int()
        _check(_LIB.dpe_state_fetch(self._ctx, int(image_id), C.byref(w), C.byref(h), None, None, None, None), "dpe_state_fetch")
        return w.value, h.value

    def state_render(self, image_id: int, kind: int, dmin: float = 0.0, dmax: float = 0.0) -> np.ndarray:
        """ShowDepthMap / ShowNormalMap / ShowWeakImage of a saved state on the device: uint8 [H, W, 3] BGR."""
        w, h = self._state_size(image_id)
        out = np.empty((h, w, 3), np.uint8)
        _check(_LIB.dpe_state_render(self._ctx, int(image_id), int(kind), float(dmin), float(dmax), out.ctypes.data),
               "dpe_state_render")
        return out

    def state_render_jpeg_blocks(self, image_id: int, kind: int, dmin: float = 0.0, dmax: float = 0.0,
                                 quality: int = 95) -> np.ndarray:
        """The picture's quantised JPEG blocks (render + front half on the device): int16 [n_blocks, 64]
        in scan order, natural coefficient order (pipeline.jpeg_blocks of the same picture)."""
        w, h = self._state_size(image_id)
        out = np.empty((((w + 15) // 16) * ((h + 15) // 16) * 6, 64), np.int16)
        _check(_LIB.dpe_state_render_jpeg_blocks(self._ctx, int(image_id), int(kind), float(dmin), float(dmax), int(quality),
                                                 out.ctypes.data, out.size, None), "dpe_state_render_jpeg_blocks")
        _check(_LIB.dpe_state_render_wait(self._ctx, out.ctypes.data), "dpe_state_render_wait")
        return out

    def viz_render_arrays(self, kind: int, depth=None, normal=None, weak=None, dmin: float = 0.0, dmax: float = 0.0) -> np.ndarray:
        """The render kernel on caller arrays (diagnostic): uint8 [H, W, 3] BGR."""
        d = None if depth is None else np.ascontiguousarray(depth, np.float32)
        n = None if normal is None else np.ascontiguousarray(normal, np.float32)
        k = None if weak is None else np.ascontiguousarray(weak, np.uint8)
        h, w = (d if d is not None else n if n is not None else k).shape[:2]
        out = np.empty((h, w, 3), np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        _check(_LIB.dpe_viz_render_arrays(self._ctx, int(kind), w, h, ptr(d), ptr(n), ptr(k), float(dmin), float(dmax),
                                          out.ctypes.data), "dpe_viz_render_arrays")
        return out

    def jpeg_blocks(self, bgr: np.ndarray, quality: int = 95) -> np.ndarray:
        """The JPEG front-half kernel on a caller uint8 [H, W, 3] BGR image (diagnostic): int16 [n_blocks, 64]."""
        a = np.ascontiguousarray(bgr, np.uint8)
        h, w = a.shape[:2]
        out = np.empty((((w + 15) // 16) * ((h + 15) // 16) * 6, 64), np.int16)
        _check(_LIB.dpe_jpeg_blocks_device(self._ctx, a.ctypes.data, w, h, int(quality), out.ctypes.data, out.size),
               "dpe_jpeg_blocks_device")
        return out

    # per-image point clouds (ExportDepthImagePointCloud; include/dpe_mvs.h)
    def state_point_cloud(self, image_id: int, mode: int, cam: _abi.DpeCamera, bgr: np.ndarray, dmin: float, dmax: float,
                          cap: int | None = None) -> np.ndarray:
        """The points f32 [n, 6] (x y z b g r) of a saved state on the device, in the reference's order; `cam`
        and `bgr` uint8 [H, W, 3] at the state's size.  `cap`: size of the point buffer (default H * W)."""
        w, h = self._state_size(image_id)
        a = np.ascontiguousarray(bgr, np.uint8)
        if a.shape != (h, w, 3):
            raise ValueError(f"expected a uint8 [{h}, {w}, 3] BGR image")
        cap = w * h if cap is None else int(cap)
        out = np.empty((max(cap, 1), 6), np.float32)
        n = C.c_size_t()
        _check(_LIB.dpe_state_point_cloud(self._ctx, int(image_id), int(mode), C.byref(cam), a.ctypes.data, float(dmin), float(dmax),
                                          out.ctypes.data, cap, C.byref(n), None), "dpe_state_point_cloud")
        _check(_LIB.dpe_state_point_cloud_wait(self._ctx, out.ctypes.data), "dpe_state_point_cloud_wait")
        return out[:n.value].copy()

    def point_cloud_arrays(self, mode: int, depth, cam: _abi.DpeCamera, bgr, dmin: float, dmax: float, weak=None,
                           cap: int | None = None) -> np.ndarray:
        """The same kernels on caller arrays (diagnostic): depth f32 [H, W], weak u8 [H, W] or None, bgr uint8 [H, W, 3]."""
        d = np.ascontiguousarray(depth, np.float32)
        h, w = d.shape
        a = np.ascontiguousarray(bgr, np.uint8)
        if a.shape != (h, w, 3):
            raise ValueError(f"expected a uint8 [{h}, {w}, 3] BGR image")
        k = None if weak is None else np.ascontiguousarray(weak, np.uint8)
        cap = w * h if cap is None else int(cap)
        out = np.empty((max(cap, 1), 6), np.float32)
        n = C.c_size_t()
        _check(_LIB.dpe_point_cloud_arrays(self._ctx, int(mode), w, h, d.ctypes.data, None if k is None else k.ctypes.data,
                                           C.byref(cam), a.ctypes.data, float(dmin), float(dmax), out.ctypes.data, cap, C.byref(n)),
               "dpe_point_cloud_arrays")
        return out[:n.value].copy()

    # cloud evaluation (include/dpe_mvs.h: dpe_cloud_nn)
    def cloud_nn(self, query, target, radius: float) -> np.ndarray:
        """out[i] = min(R*R, min_j d2(query[i], target[j])) on the device: f32 [n] SQUARED distances, the bits of
        a serial float loop (pipeline.cloud_nn gives the same on host threads).  Clouds: f32 [k, 3]."""
        q, t = as_cloud(query), as_cloud(target)
        out = np.empty(len(q), np.float32)
        _check(_LIB.dpe_cloud_nn(self._ctx, q.ctypes.data, len(q), t.ctypes.data, len(t), float(radius), out.ctypes.data),
               "dpe_cloud_nn")
        return out

    def cloud_nn_pair(self, a, b, radius: float) -> tuple:
        """Both directions with each cloud staged once: (a_to_b f32 [n], b_to_a f32 [m])."""
        a, b = as_cloud(a), as_cloud(b)
        ab, ba = np.empty(len(a), np.float32), np.empty(len(b), np.float32)
        _check(_LIB.dpe_cloud_nn_pair(self._ctx, a.ctypes.data, len(a), b.ctypes.data, len(b), float(radius), ab.ctypes.data,
                                      ba.ctypes.data), "dpe_cloud_nn_pair")
        return ab, ba

    def cloud_voxel(self, points, voxel: float, colors=None) -> tuple:
        """One record per non-empty voxel of edge `voxel` (include/dpe_mvs.h, dpe_cloud_voxel): (xyz f32 [k, 3],
        colours u8 [k, 3] or None, first i32 [k], count i32 [k]) in ascending `first`, the bits of the serial host
        loop (pipeline.voxel_down_sample).  points f32 [n, 3]; colors u8 [n, 3] or None."""
        p = as_cloud(points)
        n = len(p)
        c = None
        if colors is not None:
            c = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
            if len(c) != n:
                raise ValueError("expected one colour per point")
        xyz, first, count = np.empty((n, 3), np.float32), np.empty(n, np.int32), np.empty(n, np.int32)
        rgb = None if c is None else np.empty((n, 3), np.uint8)
        k = C.c_size_t()
        _check(_LIB.dpe_cloud_voxel(self._ctx, p.ctypes.data, n, None if c is None else c.ctypes.data, float(voxel),
                                    xyz.ctypes.data, None if rgb is None else rgb.ctypes.data, first.ctypes.data,
                                    count.ctypes.data, n, C.byref(k)), "dpe_cloud_voxel")
        k = k.value
        return xyz[:k].copy(), (None if rgb is None else rgb[:k].copy()), first[:k].copy(), count[:k].copy()

    # registration (include/dpe_mvs.h: dpe_cloud_nn_index, dpe_cloud_icp_stage, dpe_cloud_icp_step)
    def cloud_nn_index(self, query, target, radius: float) -> tuple:
        """(d2 f32 [n], idx i32 [n]): cloud_nn's distances and the index of the nearest target point, the j that
        minimises (d2, j) lexicographically, -1 where nothing is within the radius (pipeline.cloud_nn_index gives the
        same on host threads)."""
        q, t = as_cloud(query), as_cloud(target)
        d2, idx = np.empty(len(q), np.float32), np.empty(len(q), np.int32)
        _check(_LIB.dpe_cloud_nn_index(self._ctx, q.ctypes.data, len(q), t.ctypes.data, len(t), float(radius), d2.ctypes.data,
                                       idx.ctypes.data), "dpe_cloud_nn_index")
        return d2, idx

    def cloud_icp_stage(self, src, tgt, radius: float) -> None:
        """Uploads both clouds and builds the target's grid for `radius`; they stay resident for cloud_icp_step until
        the next cloud call of the context."""
        p, g = as_cloud(src), as_cloud(tgt)
        _check(_LIB.dpe_cloud_icp_stage(self._ctx, p.ctypes.data, len(p), g.ctypes.data, len(g), float(radius)), "dpe_cloud_icp_stage")

    def cloud_icp_step(self, T) -> dict:
        """One ICP step over the staged pair under T (12 numbers, 3 rows of 4): the matched count and the 16 pairwise
        sums as a dict (pipeline.cloud_icp_step gives the same bits on the host)."""
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        if t.size != 12:
            raise ValueError("expected a transform of 12 numbers (3 rows of 4)")
        s = DpeIcpSums()
        _check(_LIB.dpe_cloud_icp_step(self._ctx, t.ctypes.data, C.byref(s)), "dpe_cloud_icp_step")
        return dict(matched=int(s.matched), d2=s.d2, a=list(s.a), b=list(s.b), ab=list(s.ab))

    # depth-map evaluation (include/dpe_mvs.h: dpe_cloud_render_stage, dpe_cloud_render_view, dpe_depth_score)
    def cloud_render_stage(self, points, normals=None) -> None:
        """Uploads a scan f32 [n, 3]; it stays resident for cloud_render_view until the next cloud call of the context.
        With `normals` f32 [n, 3] (cloud_normals', or any other) the staging also serves cloud_render_view_normals."""
        p = as_cloud(points)
        if normals is None:
            _check(_LIB.dpe_cloud_render_stage(self._ctx, p.ctypes.data, len(p)), "dpe_cloud_render_stage")
            return
        nm = as_cloud(normals)
        if len(nm) != len(p):
            raise ValueError("expected one normal per point")
        _check(_LIB.dpe_cloud_render_stage_normals(self._ctx, p.ctypes.data, nm.ctypes.data, len(p)), "dpe_cloud_render_stage_normals")

    def cloud_render_view(self, cam: _abi.DpeCamera, splat: int = 0, download: bool = True):
        """The staged scan rendered into `cam` (at the map's size) with a z-buffer and a splat half-width of 0 to 8:
        f32 [height, width], the minimum depth per pixel and 0 where no point falls (pipeline.render_cloud gives the
        same bits on the host).  The map stays resident for depth_score; download=False returns None."""
        w, h = int(cam.width), int(cam.height)
        out = np.empty((max(h, 0), max(w, 0)), np.float32) if download else None
        _check(_LIB.dpe_cloud_render_view(self._ctx, C.byref(cam), int(splat), None if out is None else out.ctypes.data),
               "dpe_cloud_render_view")
        return out

    def depth_score(self, est, gt, taus, relative: bool = False, want_error: bool = False):
        """The map `est` f32 [h, w] against `gt` (None: the last rendered map) at the thresholds `taus`: the counts and
        the three pairwise sums as a dict (pipeline.score_depth gives the same bits on the host); with want_error
        (dict, error map f32 [h, w])."""
        mode = (_abi.DEPTH_TAU_REL if relative else _abi.DEPTH_TAU_ABS,)
        return self._map_score("dpe_depth_score", (), _abi.DpeDepthScore(), _abi.depth_score_dict, est, gt, taus, mode, want_error)

    def _map_score(self, entry: str, channels: tuple, s, to_dict, est, gt, taus, extra: tuple, want_error: bool):
        """depth_score and normal_score: maps of shape [h, w] + channels through the library's `entry`, whose
        arguments between the thresholds and the score struct `s` are `extra`."""
        e = np.ascontiguousarray(est, np.float32)
        if e.ndim != 2 + len(channels) or e.shape[2:] != channels:
            raise ValueError("expected a map of shape [h, w%s]" % "".join(", %d" % c for c in channels))
        g = None if gt is None else np.ascontiguousarray(gt, np.float32)
        if g is not None and g.shape != e.shape:
            raise ValueError("the maps differ in shape")
        t = np.ascontiguousarray(np.atleast_1d(taus), np.float32)
        err = np.empty(e.shape[:2], np.float32) if want_error else None
        _check(getattr(_LIB, entry)(self._ctx, e.ctypes.data, None if g is None else g.ctypes.data, e.shape[1], e.shape[0],
                                    t.ctypes.data, len(t), *extra, C.byref(s), None if err is None else err.ctypes.data), entry)
        d = to_dict(s, len(t))
        return (d, err) if want_error else d

    # normal-map evaluation (include/dpe_mvs.h: dpe_cloud_normals, dpe_cloud_render_view_normals, dpe_normal_score)
    def cloud_normals(self, points, radius: float, min_neighbours: int = 3, want_sums: bool = False) -> tuple:
        """A normal per point of the cloud f32 [n, 3] by PCA over the points within `radius` of it: (normals f32 [n, 3],
        counts i32 [n]) and with want_sums the ten integer sums i64 [n, 10] as well.  (0, 0, 0) where a point has fewer
        than min_neighbours neighbours (itself included), collinear ones, or a non-finite coordinate.  The bits of the
        host loop (pipeline.estimate_normals)."""
        p = as_cloud(points)
        n = len(p)
        normals, counts = np.empty((n, 3), np.float32), np.empty(n, np.int32)
        sums = np.empty((n, _abi.NORMAL_SUMS), np.int64) if want_sums else None
        _check(_LIB.dpe_cloud_normals(self._ctx, p.ctypes.data, n, float(radius), int(min_neighbours), normals.ctypes.data,
                                      counts.ctypes.data, None if sums is None else sums.ctypes.data), "dpe_cloud_normals")
        return (normals, counts, sums) if want_sums else (normals, counts)

    def cloud_render_view_normals(self, cam: _abi.DpeCamera, splat: int = 0, download: bool = True):
        """The staged scan and its normals rendered into `cam`: (depth f32 [height, width] with cloud_render_view's bits,
        normals f32 [height, width, 3] in the world frame, the normal of the point that wins the pixel turned towards
        the camera, zeros where there is none).  Both maps stay resident for depth_score and normal_score;
        download=False returns (None, None)."""
        w, h = int(cam.width), int(cam.height)
        depth = np.empty((max(h, 0), max(w, 0)), np.float32) if download else None
        normal = np.empty((max(h, 0), max(w, 0), 3), np.float32) if download else None
        _check(_LIB.dpe_cloud_render_view_normals(self._ctx, C.byref(cam), int(splat), None if depth is None else depth.ctypes.data,
                                                  None if normal is None else normal.ctypes.data), "dpe_cloud_render_view_normals")
        return depth, normal

    def normal_score(self, est, gt, cos_taus, want_error: bool = False):
        """The normal map `est` f32 [h, w, 3] against `gt` (None: the last rendered normal map) at the thresholds
        `cos_taus`, COSINES of the angles: the counts, the 180-bin histogram and the two pairwise sums as a dict
        (pipeline.score_normals gives the same bits on the host); with want_error (dict, error map f32 [h, w])."""
        return self._map_score("dpe_normal_score", (3,), _abi.DpeNormalScore(), _abi.normal_score_dict, est, gt, cos_taus, (), want_error)

    def cloud_timings(self) -> dict:
        """Device milliseconds of the last cloud_nn / cloud_nn_pair's parts (timing enabled), else {}.  After
        cloud_voxel the four slots are, in this order, stage, cells + insert, emit and download; after
        cloud_render_stage, cloud_render_view, cloud_render_view_normals, depth_score and normal_score stage, render,
        score and download; after cloud_normals stage, grid build, normals and download."""
        buf = (C.c_float * 4)()
        n = _LIB.dpe_cloud_last_timings(self._ctx, buf, 4)
        return {k: float(buf[i]) for i, k in enumerate(("stage", "build", "query", "download")) if i < n}

    def device_planes(self) -> int:
        return int(_LIB.dpe_pm_device_planes(self._ctx) or 0)

    def export_depth(self, dev_ptr: int, stream: int | None = None):
        _check(_LIB.dpe_pm_export_depth(self._ctx, C.c_void_p(dev_ptr), C.c_void_p(stream or 0)), "dpe_pm_export_depth")


def viz_launches() -> int:
    """Kernels of the viz medium results launched by this process so far."""
    return int(_LIB.dpe_viz_launches())


def points_launches() -> int:
    """Kernels of the per-image point clouds launched by this process so far."""
    return int(_LIB.dpe_points_launches())


def consistency_launches() -> int:
    """Kernels of the consistency maps launched by this process so far."""
    return int(_LIB.dpe_consistency_launches())


def cloud_launches() -> int:
    """Kernels of the cloud evaluation launched by this process so far."""
    return int(_LIB.dpe_cloud_launches())


def live_device_bytes() -> int:
    """Device bytes the library's contexts in this process hold at the moment."""
    return int(_LIB.dpe_live_device_bytes())


def run_pass(pass_input: dict, state: dict, device: int = 0) -> dict:
    ctx = PatchMatchContext(device)
    try:
        return ctx.run(pass_input, state)
    finally:
        ctx.close()


def param_struct(**overrides) -> _abi.DpePatchMatchParams:
    p = _abi.DpePatchMatchParams()
    _LIB.dpe_params_default(C.byref(p))
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


Context = PatchMatchContext

__all__ = ["PatchMatchContext", "Context", "viz_launches", "points_launches", "consistency_launches", "cloud_launches", "live_device_bytes", "run_pass", "param_struct", "DpeError", "LIB_PATH", "EXPORTED", "np"]
