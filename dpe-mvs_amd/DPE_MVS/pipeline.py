"""Python side of the C++ host pipeline (lib/libdpe_host.so, include/dpe_host.h).

The pipeline itself -- RunDPEPipeline / ProcessProblem / InuputInitialization, the dense_folder
I/O, the coarse-to-fine schedule, the epilogue and the .npy outputs -- is C++ (host/pipeline.cpp).
This module binds it with ctypes for what the pybind entry `DPE_MVS.dpe_mvs()` does not expose:

  * the one-process-per-GPU run from Python: `run_dpe_pipeline(..., dist=torch.distributed)` hands
    the C++ pipeline an all-gather callback (RCCL with the "nccl" backend, gloo on CPU);
  * a pass-runner hook (tests drive the C++ pipeline with the CPU oracle's runner);
  * the host helpers (grey decode, INTER_LINEAR resize, RescaleMatToTargetSize, camera reader).

It also holds writers for the dense_folder formats (.dmb, cams) used to build test datasets.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import struct

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.environ.get("DPE_HOST_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libdpe_host.so")
OUT_NAME = "DPE"
SCHEDULE_REFERENCE, SCHEDULE_JACOBI = 0, 1

ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float))


class DpePipelineOptions(C.Structure):
    _fields_ = [
        ("gpu_index", C.c_int),
        ("verbose", C.c_bool), ("fusion", C.c_bool), ("viz", C.c_bool), ("depth", C.c_bool),
        ("normal", C.c_bool), ("weak", C.c_bool), ("edge", C.c_bool),
        ("schedule", C.c_int),
        ("rank", C.c_int), ("world_size", C.c_int),
        ("allgather", ALLGATHER_FN), ("allgather_user", C.c_void_p),
        ("runner", C.c_void_p), ("runner_user", C.c_void_p),
        ("base_seed", C.c_uint64),
        ("keep_intermediate", C.c_bool),
        ("fusion_runner", C.c_void_p), ("fusion_user", C.c_void_p),
        ("max_iterations", C.c_int), ("photometric_only", C.c_bool),
        ("allgather_device", C.c_void_p), ("allgather_device_user", C.c_void_p),
        ("abort_collectives", C.c_void_p), ("abort_user", C.c_void_p),
        ("fusion_mode", C.c_int),
        ("point_cloud", C.c_int),
        ("consistency", C.c_int),
    ]


FUSION_ETH3D, FUSION_TAT_INTERMEDIATE, FUSION_TAT_ADVANCED = 0, 1, 2
FUSION_MODES = {"eth3d": FUSION_ETH3D, "tat_intermediate": FUSION_TAT_INTERMEDIATE, "tat_advanced": FUSION_TAT_ADVANCED}


POINTS_OFF, POINTS_ALL, POINTS_STRONG = 0, 1, 2
POINT_CLOUD_MODES = {"off": POINTS_OFF, "all": POINTS_ALL, "strong": POINTS_STRONG}


class DpeFusedPoint(C.Structure):   # include/dpe_mvs.h
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("b", C.c_float), ("g", C.c_float), ("r", C.c_float)]


class DpeHostTatView(C.Structure):   # include/dpe_host.h
    _fields_ = [("image_id", C.c_int), ("src_ids", C.c_void_p), ("n_src", C.c_int), ("view", _abi.DpeFusionView),
                ("bgr", C.c_void_p), ("block", C.c_void_p), ("mask", C.c_void_p)]


CLOUD_MAX_TAU = 16


class DpeCloudEval(C.Structure):   # include/dpe_host.h
    _fields_ = [("n_tau", C.c_int), ("radius", C.c_float), ("tau", C.c_float * CLOUD_MAX_TAU),
                ("precision", C.c_double * CLOUD_MAX_TAU), ("recall", C.c_double * CLOUD_MAX_TAU),
                ("fscore", C.c_double * CLOUD_MAX_TAU), ("mean_accuracy_truncated", C.c_double),
                ("mean_completeness_truncated", C.c_double), ("n_recon", C.c_ulonglong), ("n_gt", C.c_ulonglong),
                ("dropped_recon", C.c_ulonglong), ("dropped_gt", C.c_ulonglong)]


class DpeCloudPrep(C.Structure):   # include/dpe_host.h
    _fields_ = [("voxel", C.c_float), ("use_crop", C.c_int), ("crop_lo", C.c_float * 3), ("crop_hi", C.c_float * 3),
                ("n_recon_in", C.c_ulonglong), ("n_gt_in", C.c_ulonglong)]


CLOUD_MAX_RADII = 4


DpeIcpSums = _abi.DpeIcpSums   # include/dpe_mvs.h


class DpeCloudRegOptions(C.Structure):   # include/dpe_host.h
    _fields_ = [("radius", C.c_float * CLOUD_MAX_RADII), ("n_radii", C.c_int), ("max_iters", C.c_int), ("tol", C.c_double),
                ("use_init", C.c_int), ("init", C.c_double * 12)]


class DpeCloudReg(C.Structure):   # include/dpe_host.h
    _fields_ = [("T", C.c_double * 12), ("stages", C.c_int), ("iters", C.c_int * CLOUD_MAX_RADII),
                ("matched", C.c_longlong * CLOUD_MAX_RADII), ("rms", C.c_double * CLOUD_MAX_RADII),
                ("converged", C.c_int * CLOUD_MAX_RADII)]


DpeDepthScore = _abi.DpeDepthScore   # include/dpe_mvs.h
DEPTH_MAX_TAU = _abi.DEPTH_MAX_TAU


class DpeDepthStats(C.Structure):   # include/dpe_host.h
    _fields_ = [("accuracy", C.c_double * DEPTH_MAX_TAU), ("completeness", C.c_double * DEPTH_MAX_TAU), ("mae", C.c_double),
                ("mre", C.c_double), ("rmse", C.c_double)]


class DpeDepthEvalOptions(C.Structure):   # include/dpe_host.h
    _fields_ = [("dense_folder", C.c_char_p), ("map_name", C.c_char_p), ("gt_maps_dir", C.c_char_p), ("splat", C.c_int),
                ("mode", C.c_int), ("n_tau", C.c_int), ("tau", C.c_float * DEPTH_MAX_TAU), ("write_maps", C.c_int),
                ("gpu_index", C.c_int)]


class DpeDepthImage(C.Structure):   # include/dpe_host.h
    _fields_ = [("id", C.c_int), ("width", C.c_int), ("height", C.c_int), ("score", DpeDepthScore)]


DpeNormalScore = _abi.DpeNormalScore   # include/dpe_mvs.h
NORMAL_MAX_TAU = _abi.NORMAL_MAX_TAU


class DpeNormalStats(C.Structure):   # include/dpe_host.h
    _fields_ = [("share", C.c_double * NORMAL_MAX_TAU), ("completeness", C.c_double * NORMAL_MAX_TAU),
                ("mean_cos_dist", C.c_double), ("median_deg", C.c_double), ("mean_deg", C.c_double)]


class DpeNormalEvalOptions(C.Structure):   # include/dpe_host.h
    _fields_ = [("dense_folder", C.c_char_p), ("map_name", C.c_char_p), ("gt_maps_dir", C.c_char_p), ("radius", C.c_float),
                ("min_nb", C.c_int), ("splat", C.c_int), ("n_tau", C.c_int), ("cos_tau", C.c_float * NORMAL_MAX_TAU),
                ("write_maps", C.c_int), ("gpu_index", C.c_int)]


class DpeNormalImage(C.Structure):   # include/dpe_host.h
    _fields_ = [("id", C.c_int), ("width", C.c_int), ("height", C.c_int), ("score", DpeNormalScore)]


class PipelineError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError(f"host library not built: {HOST_LIB} (run `make -C dpe-mvs_amd`)")
        L = C.CDLL(HOST_LIB)
        L.dpe_pipeline_default_options.argtypes = [C.POINTER(DpePipelineOptions)]
        L.dpe_run_pipeline.argtypes = [C.c_char_p, C.POINTER(DpePipelineOptions)]
        L.dpe_run_pipeline.restype = C.c_int
        L.dpe_pipeline_last_error.restype = C.c_char_p
        L.dpe_host_read_gray.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dpe_host_read_camera.argtypes = [C.c_char_p, C.POINTER(_abi.DpeCamera)]
        L.dpe_host_resize_linear.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.dpe_host_rescale_nearest.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.dpe_host_read_bgr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dpe_host_edge_segment.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dpe_host_canny.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]
        L.dpe_host_resize_u8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.dpe_host_connect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.dpe_host_hough_lines_p.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double,
                                             C.c_double, C.c_void_p, C.c_int]
        L.dpe_host_jpeg_blocks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_size_t)]
        L.dpe_host_jpeg_write_blocks.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.dpe_host_write_jpeg.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.dpe_host_edge_segment_connect.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dpe_host_viz_render.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                          C.c_void_p]
        L.dpe_host_fusion_tat_run.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        L.dpe_host_fusion_tat_run.restype = C.c_longlong
        L.dpe_host_fusion_tat_thresholds.argtypes = [C.c_void_p, C.c_int]
        L.dpe_host_fusion_tat_angle_test.argtypes = [C.c_float, C.c_int]
        L.dpe_host_depth_point_cloud.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(_abi.DpeCamera),
                                                 C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_size_t]
        L.dpe_host_depth_point_cloud.restype = C.c_longlong
        L.dpe_host_rescale_image_and_camera.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                        C.POINTER(_abi.DpeCamera), C.c_void_p]
        L.dpe_host_write_point_cloud.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
        L.dpe_host_consistency.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.dpe_host_consistency_dot_threshold.argtypes = [C.POINTER(C.c_float)]
        L.dpe_host_consistency_angle_test.argtypes = [C.c_float]
        L.dpe_host_cloud_nn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
        L.dpe_host_read_point_cloud.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.dpe_host_cloud_eval.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_float,
                                          C.c_int, C.POINTER(DpeCloudEval)]
        L.dpe_host_cloud_voxel.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.dpe_host_cloud_crop.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
        L.dpe_host_cloud_crop.restype = C.c_size_t
        L.dpe_host_read_point_cloud_rgb.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                                    C.POINTER(C.c_int)]
        L.dpe_host_cloud_eval_prep.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_float,
                                               C.c_int, C.POINTER(DpeCloudPrep), C.POINTER(DpeCloudEval)]
        L.dpe_host_cloud_nn_index.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]
        L.dpe_host_cloud_icp_step.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p,
                                              C.POINTER(DpeIcpSums)]
        L.dpe_host_cloud_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dpe_host_cloud_solve.argtypes = [C.POINTER(DpeIcpSums), C.c_void_p, C.c_void_p, C.c_void_p]
        L.dpe_host_cloud_register.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(DpeCloudRegOptions), C.c_int,
                                              C.POINTER(DpeCloudReg)]
        L.dpe_host_cloud_eval_reg.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_float,
                                              C.c_int, C.POINTER(DpeCloudPrep), C.POINTER(DpeCloudRegOptions),
                                              C.POINTER(DpeCloudReg), C.POINTER(DpeCloudEval)]
        L.dpe_host_cloud_render.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(_abi.DpeCamera), C.c_int, C.c_void_p]
        L.dpe_host_depth_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                           C.POINTER(DpeDepthScore), C.c_void_p]
        L.dpe_host_depth_stats.argtypes = [C.POINTER(DpeDepthScore), C.c_int, C.POINTER(DpeDepthStats)]
        L.dpe_host_depth_stats.restype = None
        L.dpe_host_read_npy_f32.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dpe_host_depth_eval_list.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.dpe_host_depth_eval.argtypes = [C.POINTER(DpeDepthEvalOptions), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(DpeDepthScore)]
        L.dpe_host_cloud_normals.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dpe_host_cloud_render_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(_abi.DpeCamera), C.c_int,
                                                    C.c_void_p, C.c_void_p]
        L.dpe_host_normal_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.POINTER(DpeNormalScore), C.c_void_p]
        L.dpe_host_normal_edges.argtypes = [C.c_void_p]
        L.dpe_host_normal_edges.restype = None
        L.dpe_host_normal_cos.argtypes = [C.c_double]
        L.dpe_host_normal_cos.restype = C.c_float
        L.dpe_host_normal_stats.argtypes = [C.POINTER(DpeNormalScore), C.c_int, C.POINTER(DpeNormalStats)]
        L.dpe_host_normal_stats.restype = None
        L.dpe_host_read_npy_f32x3.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dpe_host_normal_eval.argtypes = [C.POINTER(DpeNormalEvalOptions), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_size_t), C.POINTER(DpeNormalScore)]
        _lib = L
    return _lib


# ------------------------------------------------------------------------------ host helpers (C++)
def read_gray(path: str) -> np.ndarray:
    w, h = C.c_int(), C.c_int()
    if lib().dpe_host_read_gray(path.encode(), None, 0, C.byref(w), C.byref(h)) != 0:
        raise PipelineError(f"cannot decode {path}")
    out = np.empty((h.value, w.value), np.uint8)
    lib().dpe_host_read_gray(path.encode(), out.ctypes.data, out.nbytes, C.byref(w), C.byref(h))
    return out


def read_bgr(path: str) -> np.ndarray:
    """cv::imread(path, IMREAD_COLOR): uint8 [H, W, 3] BGR."""
    w, h = C.c_int(), C.c_int()
    if lib().dpe_host_read_bgr(path.encode(), None, 0, C.byref(w), C.byref(h)) != 0:
        raise PipelineError(f"cannot decode {path}")
    out = np.empty((h.value, w.value, 3), np.uint8)
    lib().dpe_host_read_bgr(path.encode(), out.ctypes.data, out.nbytes, C.byref(w), C.byref(h))
    return out


def read_camera(path: str) -> _abi.DpeCamera:
    cam = _abi.DpeCamera()
    if lib().dpe_host_read_camera(path.encode(), C.byref(cam)) != 0:
        raise PipelineError(f"cannot read camera {path}")
    return cam


def resize_linear(img: np.ndarray, new_w: int, new_h: int) -> np.ndarray:
    src = np.ascontiguousarray(img, dtype=np.float32)
    dst = np.empty((new_h, new_w), np.float32)
    lib().dpe_host_resize_linear(src.ctypes.data, src.shape[1], src.shape[0], dst.ctypes.data, new_w, new_h)
    return dst


def rescale_to(src: np.ndarray, W: int, H: int) -> np.ndarray:
    s = np.ascontiguousarray(src)
    dst = np.zeros((H, W) + s.shape[2:], s.dtype)
    elem = s.itemsize * int(np.prod(s.shape[2:], dtype=np.int64))
    lib().dpe_host_rescale_nearest(s.ctypes.data, s.shape[1], s.shape[0], dst.ctypes.data, W, H, elem)
    return dst


# ------------------------------------------------------------------------------ viz pictures and their JPEG encoder (C++)
VIZ_DEPTH, VIZ_NORMAL, VIZ_WEAK = 0, 1, 2


def _jpeg_image(img: np.ndarray):
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError("expected a uint8 [H, W] grey or [H, W, 3] BGR image")
    return a, (1 if a.ndim == 2 else 3)


def write_jpeg(path: str, img: np.ndarray, quality: int = 95) -> None:
    """cv::imwrite(path, img) with its defaults: uint8 [H, W, 3] BGR (4:2:0) or [H, W] grey."""
    a, ch = _jpeg_image(img)
    if lib().dpe_host_write_jpeg(path.encode(), a.ctypes.data, a.shape[1], a.shape[0], ch, quality) != 0:
        raise PipelineError(f"cannot write {path}")


def jpeg_blocks(img: np.ndarray, quality: int = 95) -> np.ndarray:
    """The encoder's front half: quantised coefficient blocks int16 [n_blocks, 64], scan (MCU) order,
    natural coefficient order."""
    a, ch = _jpeg_image(img)
    n = C.c_size_t()
    if lib().dpe_host_jpeg_blocks(a.ctypes.data, a.shape[1], a.shape[0], ch, quality, None, 0, C.byref(n)) != 0:
        raise PipelineError("jpeg_blocks: bad argument")
    out = np.empty((n.value, 64), np.int16)
    if lib().dpe_host_jpeg_blocks(a.ctypes.data, a.shape[1], a.shape[0], ch, quality, out.ctypes.data, out.size, C.byref(n)) != 0:
        raise PipelineError("jpeg_blocks failed")
    return out


def write_jpeg_blocks(path: str, blocks: np.ndarray, w: int, h: int, channels: int = 3, quality: int = 95) -> None:
    """The encoder's back half: Huffman-codes `blocks` (jpeg_blocks' layout) of a w x h image into `path`."""
    b = np.ascontiguousarray(blocks, np.int16)
    if lib().dpe_host_jpeg_write_blocks(path.encode(), b.ctypes.data, w, h, channels, quality) != 0:
        raise PipelineError(f"cannot write {path}")


def viz_render(kind: int, depth=None, normal=None, weak=None, dmin: float = 0, dmax: float = 0) -> np.ndarray:
    """ShowDepthMap / ShowNormalMap / ShowWeakImage (DPE.cpp:384-502): uint8 [H, W, 3] BGR."""
    d = None if depth is None else np.ascontiguousarray(depth, np.float32)
    n = None if normal is None else np.ascontiguousarray(normal, np.float32)
    k = None if weak is None else np.ascontiguousarray(weak, np.uint8)
    src = {VIZ_DEPTH: d, VIZ_NORMAL: n, VIZ_WEAK: k}.get(kind)
    if src is None:
        raise ValueError("viz_render: bad kind or missing array")
    h, w = src.shape[:2]
    out = np.empty((h, w, 3), np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    if lib().dpe_host_viz_render(kind, w, h, ptr(d), ptr(n), ptr(k), dmin, dmax, out.ctypes.data) != 0:
        raise PipelineError("viz_render failed")
    return out


# ------------------------------------------------------------------------------ Tanks-and-Temples fusions (C++, fusion_tat.cpp)
def _fusion_mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in FUSION_MODES:
            raise ValueError(f"fusion_mode must be one of {sorted(FUSION_MODES)}, not {mode!r}")
        return FUSION_MODES[mode]
    return int(mode)


def fusion_tat_run(views, mode, gpu_index: int = -1, cap: int | None = None):
    """RunFusion_TAT_Intermediate / RunFusion_TAT_advanced (DPE.cpp:1372-1689) over `views`: dicts with
    image_id, src_ids, cam (DpeCamera), depth f32 [H, W], normal f32 [H, W, 3], bgr u8 [H, W, 3], block
    u8 [H, W] or None, in fusion order.  gpu_index < 0: the serial loops as the reference writes them;
    else the device path of the pipeline on that GPU.  `cap`: points to return at most (default: all).
    Returns (points f32 [min(n, cap), 6]: x y z b g r, masks: one u8 [H, W] per view -- filled by the
    serial loops only --, n)."""
    arr = (DpeHostTatView * len(views))()
    keep, masks, total = [], [], 0
    for k, v in enumerate(views):
        d = np.ascontiguousarray(v["depth"], np.float32)
        n = np.ascontiguousarray(v["normal"], np.float32)
        c = np.ascontiguousarray(v["bgr"], np.uint8)
        b = None if v.get("block") is None else np.ascontiguousarray(v["block"], np.uint8)
        s = np.ascontiguousarray(v["src_ids"], np.int32)
        m = np.zeros(d.shape, np.uint8)
        keep += [d, n, c, b, s]
        masks.append(m)
        total += d.size
        arr[k] = DpeHostTatView(int(v["image_id"]), s.ctypes.data, len(s),
                                _abi.DpeFusionView(d.shape[1], d.shape[0], v["cam"], d.ctypes.data, n.ctypes.data),
                                c.ctypes.data, None if b is None else b.ctypes.data, m.ctypes.data)
    cap = total if cap is None else min(cap, total)
    out = np.empty((max(cap, 1), 6), np.float32)
    cnt = lib().dpe_host_fusion_tat_run(_fusion_mode(mode), arr, len(views), gpu_index, out.ctypes.data, cap)
    if cnt < 0:
        raise PipelineError("fusion_tat_run failed (bad argument, or no such device)")
    return out[:min(cnt, cap)].copy(), masks, cnt


def fusion_tat_serial(views, mode):
    """The serial loops (the yardstick of the device path): (points f32 [n, 6], masks)."""
    pts, masks, _ = fusion_tat_run(views, mode)
    return pts, masks


def fusion_tat_thresholds(n: int = 32) -> np.ndarray:
    """D[k], k = 2..n-1: the smallest float dot product in [-1, 1] that passes the Intermediate angle
    test at k (entries 0 and 1 are unused)."""
    D = np.zeros(n, np.float32)
    if lib().dpe_host_fusion_tat_thresholds(D.ctypes.data, n) != 0:
        raise PipelineError("the angle threshold table does not verify")
    return D


def fusion_tat_angle_test(dot: float, k: int) -> bool:
    """The serial loop's angle test at k: GetAngle(dot) < k * angle_grad + angle_base."""
    return bool(lib().dpe_host_fusion_tat_angle_test(float(dot), k))


# ------------------------------------------------------------------------------ per-image point clouds (C++, points.cpp)
def _point_cloud_mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in POINT_CLOUD_MODES:
            raise ValueError(f"point_cloud must be one of {sorted(POINT_CLOUD_MODES)}, not {mode!r}")
        return POINT_CLOUD_MODES[mode]
    return int(mode)


def copy_camera(cam: _abi.DpeCamera) -> _abi.DpeCamera:
    out = _abi.DpeCamera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(_abi.DpeCamera))
    return out


def rescale_image_and_camera(bgr: np.ndarray, cam: _abi.DpeCamera, w: int, h: int):
    """RescaleImageAndCamera (DPE.cpp:1123-1144): (uint8 [h, w, 3] BGR resized per channel, a copy of `cam`
    with K[0], K[2] *= w / src_w and K[4], K[5] *= h / src_h); equal sizes give the image and K as they are."""
    a = np.ascontiguousarray(bgr, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected a uint8 [H, W, 3] BGR image")
    out, c = np.empty((h, w, 3), np.uint8), copy_camera(cam)
    if lib().dpe_host_rescale_image_and_camera(a.ctypes.data, a.shape[1], a.shape[0], w, h, C.byref(c), out.ctypes.data) != 0:
        raise PipelineError("rescale_image_and_camera: bad argument")
    return out, c


def depth_point_cloud(depth, cam: _abi.DpeCamera, bgr, depth_min: float, depth_max: float, mode=POINTS_ALL, weak=None,
                      cap: int | None = None) -> np.ndarray:
    """ExportDepthImagePointCloud (DPE.cpp:1691-1724) on the host: the points f32 [n, 6] (x y z b g r) of
    depth f32 [H, W] in the reference's order (columns outside, rows inside).  `bgr` uint8 [h, w, 3] and
    `cam` of another size go through rescale_image_and_camera first.  mode "all" / 1, or "strong" / 2
    (a pixel whose `weak` state is not STRONG gets depth 0 before the range test).  `cap`: size of the
    point buffer (default H * W); PipelineError when it is too small."""
    d = np.ascontiguousarray(depth, np.float32)
    h, w = d.shape
    k = None if weak is None else np.ascontiguousarray(weak, np.uint8)
    col, c = rescale_image_and_camera(bgr, cam, w, h)
    cap = d.size if cap is None else int(cap)
    out = np.empty((max(cap, 1), 6), np.float32)
    n = lib().dpe_host_depth_point_cloud(_point_cloud_mode(mode), w, h, d.ctypes.data, None if k is None else k.ctypes.data,
                                         C.byref(c), col.ctypes.data, depth_min, depth_max, out.ctypes.data, cap)
    if n < 0:
        raise PipelineError("depth_point_cloud failed (bad argument, or more points than cap)")
    return out[:n].copy()


def write_point_cloud(path: str, points: np.ndarray) -> None:
    """ExportPointCloud (DPE.cpp:532-572): f32 [n, 6] points (x y z b g r) as the reference's binary PLY."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 6)
    if lib().dpe_host_write_point_cloud(path.encode(), p.ctypes.data, len(p)) != 0:
        raise PipelineError(f"cannot write {path}")


# ------------------------------------------------------------------------------ consistency maps (C++, consistency.cpp)
def consistency(views, ref: int, src, min_views: int):
    """The consistency maps of reference view `ref` on the host (dpe_host_consistency): views =
    [(depth f32 [H, W], normal f32 [H, W, 3], DpeCamera)], src = indices into views.  Returns (count u8 [H, W]:
    the source views that pass RunFusion's reprojection, depth and angle tests at the pixel, without its masks,
    depth_filtered f32 [H, W]: the depth where count >= min_views, else 0)."""
    arr = (_abi.DpeFusionView * len(views))()
    keep = []
    for k, (d, n, cam) in enumerate(views):
        d = np.ascontiguousarray(d, np.float32)
        n = np.ascontiguousarray(n, np.float32)
        keep += [d, n]
        arr[k] = _abi.DpeFusionView(d.shape[1], d.shape[0], cam, d.ctypes.data, n.ctypes.data)
    s = np.ascontiguousarray(src, np.int32)
    h, w = (arr[ref].height, arr[ref].width) if 0 <= ref < len(views) else (1, 1)
    count, filtered = np.empty((h, w), np.uint8), np.empty((h, w), np.float32)
    if lib().dpe_host_consistency(arr, len(views), int(ref), s.ctypes.data, len(s), int(min_views), count.ctypes.data,
                                  filtered.ctypes.data) != 0:
        raise PipelineError("consistency: bad argument")
    return count, filtered


def consistency_dot_threshold() -> float:
    """D: the smallest float dot product in [-1, 1] whose GetAngle is below 0.174533 (the device's angle test)."""
    D = C.c_float()
    if lib().dpe_host_consistency_dot_threshold(C.byref(D)) != 0:
        raise PipelineError("the consistency angle threshold does not verify")
    return D.value


def consistency_angle_test(dot: float) -> bool:
    """The host loop's angle test: GetAngle(dot) < 0.174533f."""
    return bool(lib().dpe_host_consistency_angle_test(float(dot)))


# ------------------------------------------------------------------------------ cloud evaluation (C++, cloud_eval.cpp, ply_read.cpp)
def _last_error() -> str:
    return lib().dpe_pipeline_last_error().decode(errors="replace")


def _on_device(gpu_index: int, run, wrap_errors: bool = True):
    """run(ctx) on a context of its own on that device, closed afterwards; native.DpeError becomes PipelineError."""
    from . import native
    ctx = native.PatchMatchContext(int(gpu_index))
    try:
        return run(ctx)
    except native.DpeError as e:
        if not wrap_errors:
            raise
        raise PipelineError(str(e)) from None
    finally:
        ctx.close()


def _as_cloud(points) -> np.ndarray:
    a = np.ascontiguousarray(points, np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        if a.size:
            raise ValueError("expected points of shape [k, 3]")
        a = np.empty((0, 3), np.float32)
    return a


def read_point_cloud(path: str) -> np.ndarray:
    """The vertex positions f32 [n, 3] of a PLY (ascii or binary little-endian; x, y, z float or double at any
    position of the vertex element).  PipelineError with the reader's message for what it refuses."""
    n = C.c_size_t()
    if lib().dpe_host_read_point_cloud(os.fsencode(path), None, 0, C.byref(n)) != 0:
        raise PipelineError(_last_error())
    out = np.empty((n.value, 3), np.float32)
    if lib().dpe_host_read_point_cloud(os.fsencode(path), out.ctypes.data, n.value, C.byref(n)) != 0:
        raise PipelineError(_last_error())
    return out


def cloud_nn(query, target, radius: float) -> np.ndarray:
    """out[i] = min(R*R, min_j d2(query[i], target[j])) on host threads (dpe_host_cloud_nn): f32 [n] SQUARED
    distances, the bits of a serial float loop and of the device path (native.PatchMatchContext.cloud_nn)."""
    q, t = _as_cloud(query), _as_cloud(target)
    out = np.empty(len(q), np.float32)
    if lib().dpe_host_cloud_nn(q.ctypes.data, len(q), t.ctypes.data, len(t), float(radius), out.ctypes.data) != 0:
        raise PipelineError(_last_error())
    return out


def _as_colors(colors, n: int):
    if colors is None:
        return None
    c = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    if len(c) != n:
        raise ValueError("expected one colour per point")
    return c


def read_point_cloud_colors(path: str):
    """(positions f32 [n, 3], colours u8 [n, 3] as (b, g, r) or None) of a PLY: read_point_cloud plus the three uchar
    colour properties a PLY of ours carries (diffuse_blue / green / red, or blue / green / red)."""
    n, has = C.c_size_t(), C.c_int()
    if lib().dpe_host_read_point_cloud_rgb(os.fsencode(path), None, None, 0, C.byref(n), C.byref(has)) != 0:
        raise PipelineError(_last_error())
    xyz, rgb = np.empty((n.value, 3), np.float32), np.zeros((n.value, 3), np.uint8)
    if lib().dpe_host_read_point_cloud_rgb(os.fsencode(path), xyz.ctypes.data, rgb.ctypes.data, n.value, C.byref(n), C.byref(has)) != 0:
        raise PipelineError(_last_error())
    return xyz, (rgb if has.value else None)


def crop_cloud(points, lo, hi, colors=None):
    """(points, colours or None, original indices i32) of the finite points with lo <= p <= hi on every axis,
    compared as floats, both ends inclusive, in their order (dpe_host_cloud_crop)."""
    p = _as_cloud(points)
    c = _as_colors(colors, len(p))
    lo3, hi3 = np.ascontiguousarray(lo, np.float32).reshape(3), np.ascontiguousarray(hi, np.float32).reshape(3)
    xyz, idx = np.empty((len(p), 3), np.float32), np.empty(len(p), np.int32)
    rgb = None if c is None else np.empty((len(p), 3), np.uint8)
    k = lib().dpe_host_cloud_crop(p.ctypes.data, len(p), None if c is None else c.ctypes.data, lo3.ctypes.data, hi3.ctypes.data,
                                  xyz.ctypes.data, None if rgb is None else rgb.ctypes.data, idx.ctypes.data)
    return xyz[:k].copy(), (None if rgb is None else rgb[:k].copy()), idx[:k].copy()


def voxel_down_sample(points, voxel: float, colors=None, gpu_index: int = -1):
    """One record per non-empty voxel of edge `voxel` (include/dpe_mvs.h, dpe_cloud_voxel, states the contract):
    (xyz f32 [k, 3] lattice centroids, colours u8 [k, 3] means rounded half up or None, first i32 [k] lowest
    original index, count i32 [k]), in ascending `first`.  gpu_index < 0: the serial host loop
    (dpe_host_cloud_voxel), else native.PatchMatchContext.cloud_voxel on that device: the same bits."""
    if gpu_index >= 0:   # the device's own error, as before there was a shared helper
        return _on_device(gpu_index, lambda ctx: ctx.cloud_voxel(points, voxel, colors), wrap_errors=False)
    p = _as_cloud(points)
    c = _as_colors(colors, len(p))
    n = len(p)
    xyz, first, count = np.empty((n, 3), np.float32), np.empty(n, np.int32), np.empty(n, np.int32)
    rgb = None if c is None else np.empty((n, 3), np.uint8)
    k = C.c_size_t()
    if lib().dpe_host_cloud_voxel(p.ctypes.data, n, None if c is None else c.ctypes.data, float(voxel), xyz.ctypes.data,
                                  None if rgb is None else rgb.ctypes.data, first.ctypes.data, count.ctypes.data, n, C.byref(k)) != 0:
        raise PipelineError(_last_error())
    k = k.value
    return xyz[:k].copy(), (None if rgb is None else rgb[:k].copy()), first[:k].copy(), count[:k].copy()


# ------------------------------------------------------------------------------ registration (C++, cloud_register.cpp)
def cloud_nn_index(query, target, radius: float):
    """(d2 f32 [n], idx i32 [n]) on host threads (dpe_host_cloud_nn_index): cloud_nn's distances and the index of the
    nearest target point, the j that minimises (d2, j) lexicographically, -1 where nothing is within the radius: the
    bits of the device path (native.PatchMatchContext.cloud_nn_index)."""
    q, t = _as_cloud(query), _as_cloud(target)
    d2, idx = np.empty(len(q), np.float32), np.empty(len(q), np.int32)
    if lib().dpe_host_cloud_nn_index(q.ctypes.data, len(q), t.ctypes.data, len(t), float(radius), d2.ctypes.data, idx.ctypes.data) != 0:
        raise PipelineError(_last_error())
    return d2, idx


def _as_transform(T) -> np.ndarray:
    t = np.ascontiguousarray(T, np.float64).reshape(-1)
    if t.size != 12:
        raise ValueError("expected a transform of 12 numbers (3 rows of 4)")
    return t


def icp_sums_dict(s: DpeIcpSums) -> dict:
    return dict(matched=int(s.matched), d2=s.d2, a=list(s.a), b=list(s.b), ab=list(s.ab))


def cloud_icp_step(src, tgt, radius: float, T) -> dict:
    """One ICP step on the host (dpe_host_cloud_icp_step; include/dpe_mvs.h states it): the matched count and the 16
    pairwise sums d2, a[3], b[3], ab[9] as a dict, the bits of the device step."""
    p, g, t = _as_cloud(src), _as_cloud(tgt), _as_transform(T)
    s = DpeIcpSums()
    if lib().dpe_host_cloud_icp_step(p.ctypes.data, len(p), g.ctypes.data, len(g), float(radius), t.ctypes.data, C.byref(s)) != 0:
        raise PipelineError(_last_error())
    return icp_sums_dict(s)


def cloud_solve(sums: dict, o_s, o_t) -> np.ndarray:
    """The transform f64 [3, 4] of the original source points from one step's sums (dpe_host_cloud_solve); o_s and
    o_t are the per-axis minima of the finite points of the source and the target."""
    s = DpeIcpSums(int(sums["matched"]), float(sums["d2"]), (C.c_double * 3)(*sums["a"]), (C.c_double * 3)(*sums["b"]),
                   (C.c_double * 9)(*sums["ab"]))
    a, b = np.ascontiguousarray(o_s, np.float64).reshape(3), np.ascontiguousarray(o_t, np.float64).reshape(3)
    T = np.empty(12, np.float64)
    if lib().dpe_host_cloud_solve(C.byref(s), a.ctypes.data, b.ctypes.data, T.ctypes.data) != 0:
        raise PipelineError(_last_error())
    return T.reshape(3, 4)


def transform_cloud(T, points) -> np.ndarray:
    """points f32 [n, 3] under T (3 rows of 4, [R | t]) in the step's own expression (dpe_host_cloud_transform):
    (float)(((T0 x + T1 y) + T2 z) + T3) per row in double; a non-finite point becomes NaN."""
    p, t = _as_cloud(points), _as_transform(T)
    out = np.empty_like(p)
    if lib().dpe_host_cloud_transform(t.ctypes.data, p.ctypes.data, len(p), out.ctypes.data) != 0:
        raise PipelineError(_last_error())
    return out


def _reg_options(radii, max_iters: int = 50, tol: float = 1e-6, init=None) -> DpeCloudRegOptions:
    o = DpeCloudRegOptions()
    r = [float(v) for v in np.atleast_1d(radii)]
    o.n_radii = len(r)
    for k, v in enumerate(r[:CLOUD_MAX_RADII]):
        o.radius[k] = v
    o.max_iters, o.tol = int(max_iters), float(tol)
    if init is not None:
        o.use_init = 1
        o.init[:] = list(_as_transform(init))
    return o


def _reg_dict(r: DpeCloudReg, o: DpeCloudRegOptions) -> dict:
    return dict(T=[[r.T[4 * i + j] for j in range(4)] for i in range(3)],
                stages=[dict(radius=float(o.radius[k]), iters=int(r.iters[k]), matched=int(r.matched[k]), rms=r.rms[k],
                             converged=int(r.converged[k])) for k in range(r.stages)])


def register_clouds(src, tgt, radii, max_iters: int = 50, tol: float = 1e-6, init=None, gpu_index: int = -1) -> dict:
    """Rigid registration of cloud `src` onto cloud `tgt` by point-to-point ICP (dpe_host_cloud_register;
    include/dpe_host.h states the loop): `radii` is one match radius or 1 to 4 of them, coarse to fine, each run for
    at most `max_iters` steps; `init` a starting transform (3 rows of 4; default the identity).  gpu_index < 0: the
    host step, else the device step on that device: equal dicts.  Returns T (3 rows of 4, to be applied with
    transform_cloud) and per stage radius, iters, matched, rms and converged (2: a fixed point, 1: rms within tol,
    0: max_iters)."""
    p, g = _as_cloud(src), _as_cloud(tgt)
    o = _reg_options(radii, max_iters, tol, init)
    r = DpeCloudReg()
    if lib().dpe_host_cloud_register(p.ctypes.data, len(p), g.ctypes.data, len(g), C.byref(o), int(gpu_index), C.byref(r)) != 0:
        raise PipelineError(_last_error())
    return _reg_dict(r, o)


def evaluate_clouds(recon, gt, taus, radius: float | None = None, gpu_index: int = -1, voxel: float | None = None,
                    crop=None, register=None) -> dict:
    """Precision, recall and F-score of cloud `recon` against cloud `gt` (f32 [k, 3]) at the thresholds `taus`
    (1 to 16, each 0 < tau <= radius; radius None: the largest tau), from the truncated nearest-neighbour
    distances in both directions (dpe_host_cloud_eval).  gpu_index < 0: on host threads, else on that device:
    equal dicts.  Keys: tau, precision, recall, fscore (lists), radius, mean_accuracy_truncated,
    mean_completeness_truncated (means of the distances truncated at the radius), n_recon, n_gt, dropped_recon,
    dropped_gt (points with a non-finite coordinate; they still count in the denominators).
    `crop` = (lo, hi) keeps the points of both clouds inside that box first, `voxel` then down-samples both to one
    point per voxel (voxel_down_sample; on the device too when gpu_index >= 0) before they are scored
    (dpe_host_cloud_eval_prep).  With either the dict also has voxel (or None), crop ([lo, hi] or None), n_recon_in and
    n_gt_in (the counts before the preparation; n_recon and n_gt are those after it).
    `register` = a radius, a list of radii or a dict of register_clouds' options (radii, max_iters, tol, init) first
    moves the reconstruction onto the ground truth (dpe_host_cloud_eval_reg: the down-sampled copies are registered,
    the ground truth cropped, then the whole reconstruction is transformed and scored as above); the dict then has
    `registration`, register_clouds' dict."""
    a, b = _as_cloud(recon), _as_cloud(gt)
    t = np.ascontiguousarray(np.atleast_1d(taus), np.float32)
    e = DpeCloudEval()
    prep = None
    if voxel is not None or crop is not None:
        prep = DpeCloudPrep()
        prep.voxel = 0.0 if voxel is None else float(voxel)
        if voxel is not None and not prep.voxel > 0.0:
            raise PipelineError("cloud_eval: the voxel edge is not a finite positive number")
        if crop is not None:
            prep.use_crop = 1
            for k in range(3):
                prep.crop_lo[k], prep.crop_hi[k] = float(crop[0][k]), float(crop[1][k])
    R = 0.0 if radius is None else float(radius)
    if register is None:
        rc = lib().dpe_host_cloud_eval_prep(a.ctypes.data, len(a), b.ctypes.data, len(b), t.ctypes.data, len(t), R, int(gpu_index),
                                            None if prep is None else C.byref(prep), C.byref(e))
    else:
        ropt = _reg_options(**register) if isinstance(register, dict) else _reg_options(register)
        reg = DpeCloudReg()
        rc = lib().dpe_host_cloud_eval_reg(a.ctypes.data, len(a), b.ctypes.data, len(b), t.ctypes.data, len(t), R, int(gpu_index),
                                           None if prep is None else C.byref(prep), C.byref(ropt), C.byref(reg), C.byref(e))
    if rc != 0:
        raise PipelineError(_last_error())
    k = e.n_tau
    out = _cloud_eval_dict(e, k)
    if register is not None:
        out["registration"] = _reg_dict(reg, ropt)
    if prep is not None:
        out.update(voxel=(float(prep.voxel) if voxel is not None else None),
                   crop=([[float(v) for v in prep.crop_lo], [float(v) for v in prep.crop_hi]] if crop is not None else None),
                   n_recon_in=int(prep.n_recon_in), n_gt_in=int(prep.n_gt_in))
    return out


def _cloud_eval_dict(e: DpeCloudEval, k: int) -> dict:
    return dict(tau=[float(v) for v in e.tau[:k]], precision=list(e.precision[:k]), recall=list(e.recall[:k]),
                fscore=list(e.fscore[:k]), radius=float(e.radius), mean_accuracy_truncated=e.mean_accuracy_truncated,
                mean_completeness_truncated=e.mean_completeness_truncated, n_recon=int(e.n_recon), n_gt=int(e.n_gt),
                dropped_recon=int(e.dropped_recon), dropped_gt=int(e.dropped_gt))


def format_cloud_eval(e: dict) -> str:
    """The table bin/dpe_eval prints, from evaluate_clouds' dict."""
    rows = []
    if "registration" in e:
        st = e["registration"]["stages"]
        rows.append("registered: radii %s, rms %.9g" % (" ".join("%.9g" % s["radius"] for s in st), st[-1]["rms"]))
        rows += ["T %.17g %.17g %.17g %.17g" % tuple(row) for row in e["registration"]["T"]]
    if "n_recon_in" in e:
        box = "none" if e["crop"] is None else "[%.9g %.9g %.9g] to [%.9g %.9g %.9g]" % tuple(e["crop"][0] + e["crop"][1])
        rows.append("prepared: voxel %.9g, crop %s, from recon %d points, gt %d points"
                    % (e["voxel"] or 0.0, box, e["n_recon_in"], e["n_gt_in"]))
    rows += ["recon %d points (%d dropped), gt %d points (%d dropped), radius %.9g"
            % (e["n_recon"], e["dropped_recon"], e["n_gt"], e["dropped_gt"], e["radius"]),
            "%14s %10s %10s %10s" % ("tau", "precision", "recall", "fscore")]
    rows += ["%14.9g %10.6f %10.6f %10.6f" % v for v in zip(e["tau"], e["precision"], e["recall"], e["fscore"])]
    rows += ["mean accuracy (truncated at the radius) %.9g" % e["mean_accuracy_truncated"],
             "mean completeness (truncated at the radius) %.9g" % e["mean_completeness_truncated"]]
    return "\n".join(rows) + "\n"


# ------------------------------------------------------------------------------ what the two map evaluations share
def _read_npy(entry, path: str, channels: tuple) -> np.ndarray:
    """A dpe_host_read_npy_* entry in its two calls: the size, then the values into f32 [h, w] + channels."""
    w, h = C.c_int(), C.c_int()
    if entry(os.fsencode(path), None, 0, C.byref(w), C.byref(h)) != 0:
        raise PipelineError(_last_error())
    out = np.empty((h.value, w.value) + channels, np.float32)
    if entry(os.fsencode(path), out.ctypes.data, out.size, C.byref(w), C.byref(h)) != 0:
        raise PipelineError(_last_error())
    return out


def _score_struct(s, score: dict, sums: tuple):
    """The score struct `s` filled from a score's dict: the counts, the named sums, within[] and, where it has one, hist[]."""
    for name in ("n_px", "n_gt", "n_est", "n_both") + sums:
        setattr(s, name, score[name])
    for name in ("within", "hist"):
        for i, v in enumerate(score.get(name, ())):
            getattr(s, name)[i] = v
    return s


def _format_map_eval(e: dict, first: str, col_fmt: str, cols: tuple, row_fmt: str, keys: tuple, share: str, share_key: str) -> str:
    """The table of a folder evaluation: the line `first`, the header (the metric's three columns `cols`, then
    `share`[k] and comp[k] per threshold), a row per image and the total."""
    k = len(e["total"]["within"])
    rows = [first, ("%8s %11s %10s %10s %10s" + col_fmt) % (("image", "size", "n_gt", "n_est", "n_both") + cols)
            + "".join(" %10s %10s" % ("%s[%d]" % (share, i), "comp[%d]" % i) for i in range(k))]

    def row(name, size, s):
        return (("%8s %11s %10d %10d %10d" + row_fmt) % ((name, size, s["n_gt"], s["n_est"], s["n_both"]) + tuple(s[n] for n in keys))
                + "".join(" %10.6f %10.6f" % v for v in zip(s[share_key], s["completeness"])))

    rows += [row("%08d" % s["id"], "%dx%d" % (s["width"], s["height"]), s) for s in e["images"]]
    rows.append(row("total", "-", e["total"]))
    return "\n".join(rows) + "\n"


# ------------------------------------------------------------------------------ depth-map evaluation (C++, depth_eval.cpp)
def read_npy_f32(path: str) -> np.ndarray:
    """A 2-D '<f4' .npy v1.0 in C order through the host library's reader (dpe_host_read_npy_f32): f32 [h, w].
    PipelineError with the reader's message for what it refuses (another dtype, rank or order, a body that is
    shorter or longer than the header says)."""
    return _read_npy(lib().dpe_host_read_npy_f32, path, ())


def render_cloud(points, cam: _abi.DpeCamera, splat: int = 0, gpu_index: int = -1) -> np.ndarray:
    """The scan `points` f32 [n, 3] rendered into `cam` (a camera at the map's size) with a z-buffer: f32
    [height, width], per pixel the minimum depth of the points whose (2 splat + 1)^2 pixels cover it, 0 where none
    does (include/dpe_mvs.h, dpe_cloud_render_view, states the contract; no occlusion test beyond the z-buffer).
    gpu_index < 0: the host loop (dpe_host_cloud_render), else on that device: the same bits."""
    if gpu_index >= 0:
        return _on_device(gpu_index, lambda ctx: (ctx.cloud_render_stage(points), ctx.cloud_render_view(cam, splat))[1])
    p = _as_cloud(points)
    out = np.empty((max(int(cam.height), 0), max(int(cam.width), 0)), np.float32)
    if lib().dpe_host_cloud_render(p.ctypes.data, len(p), C.byref(cam), int(splat), out.ctypes.data) != 0:
        raise PipelineError(_last_error())
    return out


def depth_stats(score: dict) -> dict:
    """What is derived from a score's counts and sums, in double (dpe_host_depth_stats, the one function both paths
    and both programs go through): accuracy and completeness per threshold, mae, mre, rmse; 0 for an empty
    denominator."""
    s, d = _score_struct(DpeDepthScore(), score, ("sum_abs", "sum_rel", "sum_sq")), DpeDepthStats()
    k = len(score["within"])
    lib().dpe_host_depth_stats(C.byref(s), k, C.byref(d))
    return dict(accuracy=list(d.accuracy[:k]), completeness=list(d.completeness[:k]), mae=d.mae, mre=d.mre, rmse=d.rmse)


def _depth_dict(s: DpeDepthScore, k: int) -> dict:
    d = _abi.depth_score_dict(s, k)
    d.update(depth_stats(d))
    return d


def score_depth(est, gt, taus, relative: bool = False, gpu_index: int = -1, want_error: bool = False):
    """The depth map `est` against the ground-truth map `gt` (f32 [h, w]) at the thresholds `taus` (1 to 16, each
    finite and >= 0; relative: |est - gt| < tau * gt instead of < tau).  A dict of the counts n_px, n_gt, n_est,
    n_both, within[k], the pairwise sums sum_abs, sum_rel, sum_sq (include/dpe_mvs.h, dpe_depth_score) and
    depth_stats of them.  gpu_index < 0: the host loop (dpe_host_depth_score), else on that device: equal dicts.
    want_error: (dict, error map f32 [h, w]: the error where both are usable, -1 where only gt is, else -2)."""
    t = np.ascontiguousarray(np.atleast_1d(taus), np.float32)
    e, g = np.ascontiguousarray(est, np.float32), np.ascontiguousarray(gt, np.float32)
    if e.ndim != 2 or g.shape != e.shape:
        raise PipelineError("depth_score: size mismatch: two maps of one shape [h, w] expected")
    if gpu_index >= 0:
        r = _on_device(gpu_index, lambda ctx: ctx.depth_score(e, g, t, relative, want_error))
        d, err = r if want_error else (r, None)
        d.update(depth_stats(d))
        return (d, err) if want_error else d
    s = DpeDepthScore()
    err = np.empty(e.shape, np.float32) if want_error else None
    if lib().dpe_host_depth_score(e.ctypes.data, g.ctypes.data, e.shape[1], e.shape[0], t.ctypes.data, len(t),
                                  _abi.DEPTH_TAU_REL if relative else _abi.DEPTH_TAU_ABS, C.byref(s),
                                  None if err is None else err.ctypes.data) != 0:
        raise PipelineError(_last_error())
    d = _depth_dict(s, len(t))
    return (d, err) if want_error else d


def evaluate_depth_maps(dense_folder: str, gt, taus, relative: bool = False, splat: int = 0, map_name: str = "depth.npy",
                        gt_maps: str | None = None, write_maps: bool = False, gpu_index: int = -1) -> dict:
    """The depth maps DPE/%08d/<map_name> of a dense folder, in ascending image id, against the scan `gt` (f32
    [n, 3]) rendered into each cams/%08d_cam.txt at the map's size (render_cloud, half-width `splat`), or, with
    gt_maps = a folder, against its %08d.npy (dpe_host_depth_eval).  write_maps also writes depth_gt.npy and
    depth_error.npy beside each map.  gpu_index < 0: on the host, else the scan is staged once on that device and
    every view rendered and scored there: equal dicts.  Keys: map, relative, splat, tau, n_gt_points, images (a
    list of score_depth's dicts with id, width, height) and total (the counts added, the sums added in ascending
    id, and depth_stats of them)."""
    t = np.ascontiguousarray(np.atleast_1d(taus), np.float32)
    if len(t) < 1 or len(t) > DEPTH_MAX_TAU:
        raise PipelineError("depth_score: 1 to 16 thresholds expected")
    if gt is None and gt_maps is None:
        raise PipelineError("depth_eval: a scan or a folder of ground-truth maps expected")
    p = _as_cloud(np.empty((0, 3), np.float32) if gt is None else gt)
    o = DpeDepthEvalOptions()
    o.dense_folder, o.map_name = os.fsencode(dense_folder), os.fsencode(map_name)
    o.gt_maps_dir = None if gt_maps is None else os.fsencode(gt_maps)
    o.splat, o.mode, o.n_tau = int(splat), (_abi.DEPTH_TAU_REL if relative else _abi.DEPTH_TAU_ABS), len(t)
    for k, v in enumerate(t):
        o.tau[k] = v
    o.write_maps, o.gpu_index = int(bool(write_maps)), int(gpu_index)
    n = C.c_size_t()
    if lib().dpe_host_depth_eval_list(o.dense_folder, o.map_name, None, 0, C.byref(n)) != 0:
        raise PipelineError(_last_error())
    rows, total = (DpeDepthImage * n.value)(), DpeDepthScore()
    if lib().dpe_host_depth_eval(C.byref(o), p.ctypes.data, len(p), rows, n.value, C.byref(n), C.byref(total)) != 0:
        raise PipelineError(_last_error())
    images = [dict(_depth_dict(r.score, len(t)), id=int(r.id), width=int(r.width), height=int(r.height)) for r in rows[:n.value]]
    return dict(map=map_name, relative=bool(relative), splat=int(splat), tau=[float(v) for v in t],
                n_gt_points=(None if gt_maps is not None else len(p)), images=images, total=_depth_dict(total, len(t)))


def format_depth_eval(e: dict) -> str:
    """The table bin/dpe_depth_eval prints, from evaluate_depth_maps' dict."""
    gt = "maps" if e["n_gt_points"] is None else "cloud of %d points, splat %d" % (e["n_gt_points"], e["splat"])
    first = "map %s, ground truth %s, %s thresholds %s" % (e["map"], gt, "relative" if e["relative"] else "absolute",
                                                          " ".join("%.9g" % v for v in e["tau"]))
    return _format_map_eval(e, first, " %12s %12s %12s", ("mae", "mre", "rmse"), " %12.6g %12.6g %12.6g", ("mae", "mre", "rmse"),
                            "acc", "accuracy")


# ------------------------------------------------------------------------------ normal-map evaluation (C++, normal_eval.cpp)
def read_npy_f32x3(path: str) -> np.ndarray:
    """A 3-D '<f4' .npy v1.0 in C order of shape [h, w, 3] through the host library's reader
    (dpe_host_read_npy_f32x3): f32 [h, w, 3].  PipelineError with the reader's message for what it refuses."""
    return _read_npy(lib().dpe_host_read_npy_f32x3, path, (3,))


def normal_edges() -> np.ndarray:
    """The 180 bin edges of the score's histogram, E[b] = (float)cos(b degrees): the table both paths use."""
    e = np.empty(_abi.NORMAL_BINS, np.float32)
    lib().dpe_host_normal_edges(e.ctypes.data)
    return e


def normal_cos(deg: float) -> float:
    """A threshold in degrees as the cosine the score takes (dpe_host_normal_cos, the one place where this happens)."""
    return float(lib().dpe_host_normal_cos(float(deg)))


def estimate_normals(points, radius: float, min_neighbours: int = 3, gpu_index: int = -1, want_sums: bool = False) -> tuple:
    """A normal per point of the cloud f32 [n, 3] by PCA over the points within `radius` of it (include/dpe_mvs.h,
    dpe_cloud_normals, states the contract): (normals f32 [n, 3], counts i32 [n]), with want_sums also the ten integer
    sums i64 [n, 10].  (0, 0, 0) = no normal: fewer than min_neighbours neighbours (the point itself counts),
    collinear neighbours, or a non-finite point.  The sign makes the component of largest magnitude positive; a view
    turns it towards its camera (render_cloud_normals).  gpu_index < 0: on host threads (dpe_host_cloud_normals), else
    on that device: the same bits."""
    if gpu_index >= 0:
        return _on_device(gpu_index, lambda ctx: ctx.cloud_normals(points, radius, min_neighbours, want_sums))
    p = _as_cloud(points)
    n = len(p)
    normals, counts = np.empty((n, 3), np.float32), np.empty(n, np.int32)
    sums = np.empty((n, _abi.NORMAL_SUMS), np.int64) if want_sums else None
    if lib().dpe_host_cloud_normals(p.ctypes.data, n, float(radius), int(min_neighbours), normals.ctypes.data, counts.ctypes.data,
                                    None if sums is None else sums.ctypes.data) != 0:
        raise PipelineError(_last_error())
    return (normals, counts, sums) if want_sums else (normals, counts)


def render_cloud_normals(points, normals, cam: _abi.DpeCamera, splat: int = 0, gpu_index: int = -1) -> tuple:
    """The scan `points` and its per-point `normals` (both f32 [n, 3]) rendered into `cam`: (depth f32 [height, width],
    render_cloud's bits, normal map f32 [height, width, 3] in the world frame).  A pixel takes the normal of the point
    that wins its z-buffer (the lexicographic minimum of depth bits and index), turned towards the camera; zeros where
    no point falls or the winner has no normal.  gpu_index < 0: the host loop, else on that device: the same bits."""
    p, nm = _as_cloud(points), _as_cloud(normals)
    if len(p) != len(nm):
        raise PipelineError("cloud_render_normals: one normal per point expected")
    if gpu_index >= 0:
        return _on_device(gpu_index, lambda ctx: (ctx.cloud_render_stage(p, nm), ctx.cloud_render_view_normals(cam, splat))[1])
    h, w = max(int(cam.height), 0), max(int(cam.width), 0)
    depth, normal = np.empty((h, w), np.float32), np.empty((h, w, 3), np.float32)
    if lib().dpe_host_cloud_render_normals(p.ctypes.data, nm.ctypes.data, len(p), C.byref(cam), int(splat), depth.ctypes.data,
                                           normal.ctypes.data) != 0:
        raise PipelineError(_last_error())
    return depth, normal


def normal_stats(score: dict) -> dict:
    """What is derived from a score's counts, histogram and sums, in double (dpe_host_normal_stats, the one function
    both paths and both programs go through): share and completeness per threshold, mean_cos_dist, and median_deg
    and mean_deg from the histogram to its 1 degree resolution; 0 for an empty denominator."""
    s, d = _score_struct(DpeNormalScore(), score, ("sum_dist", "sum_dist_sq")), DpeNormalStats()
    k = len(score["within"])
    lib().dpe_host_normal_stats(C.byref(s), k, C.byref(d))
    return dict(share=list(d.share[:k]), completeness=list(d.completeness[:k]), mean_cos_dist=d.mean_cos_dist,
                median_deg=d.median_deg, mean_deg=d.mean_deg)


def _normal_dict(s: DpeNormalScore, k: int) -> dict:
    d = _abi.normal_score_dict(s, k)
    d.update(normal_stats(d))
    return d


def score_normals(est, gt, taus_deg=None, cos_taus=None, gpu_index: int = -1, want_error: bool = False):
    """The normal map `est` against the ground-truth map `gt` (f32 [h, w, 3]) at 1 to 16 thresholds, angles in degrees
    (taus_deg, turned into cosines by normal_cos) or their cosines directly (cos_taus).  A dict of the counts n_px,
    n_gt, n_est, n_both, within[k], the histogram hist[180] of the angle in degrees, the pairwise sums sum_dist and
    sum_dist_sq of 1 - cos (include/dpe_mvs.h, dpe_normal_score) and normal_stats of them.  A pixel counts where both
    maps hold a finite non-zero vector; the vectors need not be unit.  gpu_index < 0: the host loop, else on that
    device: equal dicts.  want_error: (dict, error map f32 [h, w]: the cosine where both have a normal, -2 where only
    gt has, else -3)."""
    if (taus_deg is None) == (cos_taus is None):
        raise PipelineError("normal_score: thresholds in degrees or as cosines expected, not both")
    t = (np.ascontiguousarray(np.atleast_1d(cos_taus), np.float32) if cos_taus is not None
         else np.array([normal_cos(v) for v in np.atleast_1d(taus_deg)], np.float32))
    e, g = np.ascontiguousarray(est, np.float32), np.ascontiguousarray(gt, np.float32)
    if e.ndim != 3 or e.shape[2] != 3 or g.shape != e.shape:
        raise PipelineError("normal_score: size mismatch: two maps of one shape [h, w, 3] expected")
    if gpu_index >= 0:
        r = _on_device(gpu_index, lambda ctx: ctx.normal_score(e, g, t, want_error))
        d, err = r if want_error else (r, None)
        d.update(normal_stats(d))
        return (d, err) if want_error else d
    s = DpeNormalScore()
    err = np.empty(e.shape[:2], np.float32) if want_error else None
    if lib().dpe_host_normal_score(e.ctypes.data, g.ctypes.data, e.shape[1], e.shape[0], t.ctypes.data, len(t), C.byref(s),
                                   None if err is None else err.ctypes.data) != 0:
        raise PipelineError(_last_error())
    d = _normal_dict(s, len(t))
    return (d, err) if want_error else d


def evaluate_normal_maps(dense_folder: str, gt, radius, taus_deg, min_neighbours: int = 3, splat: int = 0,
                         gt_normals: str | None = None, write_maps: bool = False, gpu_index: int = -1) -> dict:
    """The normal maps DPE/%08d/normal.npy of a dense folder, in ascending image id, against the scan `gt` (f32
    [n, 3]): its normals are estimated once (estimate_normals: radius, min_neighbours) and rendered into each
    cams/%08d_cam.txt at the map's size (render_cloud_normals, half-width `splat`); or, with gt_normals = a folder,
    against its %08d.npy [h, w, 3] (dpe_host_normal_eval).  write_maps also writes normal_gt.npy and normal_error.npy
    beside each map.  gpu_index < 0: on the host, else everything in one context of that device: equal dicts.
    Keys: map, radius, min_neighbours, splat, tau_deg, n_gt_points, images (a list of score_normals' dicts with id,
    width, height) and total (the counts added, the sums added in ascending id, and normal_stats of them)."""
    deg = [float(v) for v in np.atleast_1d(taus_deg)]
    if len(deg) < 1 or len(deg) > NORMAL_MAX_TAU:
        raise PipelineError("normal_score: 1 to 16 thresholds expected")
    if gt is None and gt_normals is None:
        raise PipelineError("normal_eval: a scan or a folder of ground-truth normal maps expected")
    p = _as_cloud(np.empty((0, 3), np.float32) if gt is None else gt)
    o = DpeNormalEvalOptions()
    o.dense_folder, o.map_name = os.fsencode(dense_folder), None
    o.gt_maps_dir = None if gt_normals is None else os.fsencode(gt_normals)
    o.radius = 0.0 if radius is None else float(radius)
    o.min_nb, o.splat, o.n_tau = int(min_neighbours), int(splat), len(deg)
    for k, v in enumerate(deg):
        o.cos_tau[k] = normal_cos(v)
    o.write_maps, o.gpu_index = int(bool(write_maps)), int(gpu_index)
    n = C.c_size_t()
    if lib().dpe_host_depth_eval_list(o.dense_folder, b"normal.npy", None, 0, C.byref(n)) != 0:
        n = C.c_size_t(0)   # dpe_host_normal_eval lists again and reports what it refuses in its own words
    rows, total = (DpeNormalImage * max(n.value, 1))(), DpeNormalScore()
    if lib().dpe_host_normal_eval(C.byref(o), p.ctypes.data, len(p), rows, n.value, C.byref(n), C.byref(total)) != 0:
        raise PipelineError(_last_error())
    k = len(deg)
    images = [dict(_normal_dict(r.score, k), id=int(r.id), width=int(r.width), height=int(r.height)) for r in rows[:n.value]]
    return dict(map="normal.npy", radius=(None if gt_normals is not None else float(np.float32(o.radius))),
                min_neighbours=int(min_neighbours), splat=int(splat), tau_deg=[float(np.float32(v)) for v in deg],
                n_gt_points=(None if gt_normals is not None else len(p)), images=images, total=_normal_dict(total, k))


def format_normal_eval(e: dict) -> str:
    """The table bin/dpe_normal_eval prints, from evaluate_normal_maps' dict."""
    gt = "maps" if e["n_gt_points"] is None else "cloud of %d points, radius %.9g, min neighbours %d, splat %d" % (
        e["n_gt_points"], e["radius"], e["min_neighbours"], e["splat"])
    first = "map %s, ground truth %s, thresholds in degrees %s" % (e["map"], gt, " ".join("%.9g" % v for v in e["tau_deg"]))
    return _format_map_eval(e, first, " %12s %10s %10s", ("cos_dist", "median", "mean"), " %12.6g %10.1f %10.4f",
                            ("mean_cos_dist", "median_deg", "mean_deg"), "within", "share")


# ------------------------------------------------------------------------------ EdgeSegment (C++, edges.cpp)
def _u8(img: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("expected a 2-D uint8 image")
    return a


def edge_segment(scale: int, img: np.ndarray, mode: int, use_canny: bool, high_res: bool = True) -> np.ndarray:
    """EdgeSegment (DPE.cpp:129-291): mode 0 -> uint8 0/255 edges, mode 1 -> int32 labels."""
    a = _u8(img)
    ow, oh = C.c_int(), C.c_int()
    args = (scale, a.ctypes.data, a.shape[1], a.shape[0], mode, int(use_canny), int(high_res))
    if lib().dpe_host_edge_segment(*args, None, 0, C.byref(ow), C.byref(oh)) != 0:
        raise PipelineError("EdgeSegment failed")
    out = np.empty((oh.value, ow.value), np.uint8 if mode == 0 else np.int32)
    if lib().dpe_host_edge_segment(*args, out.ctypes.data, out.nbytes, C.byref(ow), C.byref(oh)) != 0:
        raise PipelineError("EdgeSegment failed")
    return out


def connect_color(label: int):
    """colors[label] of connect_<s>.jpg as (B, G, R): a fixed 32-bit hash of the label, label 0 black."""
    if label == 0:
        return (0, 0, 0)
    x = label & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return (x & 255, (x >> 8) & 255, (x >> 16) & 255)


def edge_segment_connect(scale: int, img: np.ndarray, high_res: bool = True):
    """EdgeSegment's labels (mode 1) and its img_connect picture (uint8 [h, w, 3] BGR: colors[label] before
    the small regions become -1) from one segmentation."""
    a = _u8(img)
    ow, oh = C.c_int(), C.c_int()
    args = (scale, a.ctypes.data, a.shape[1], a.shape[0], int(high_res))
    if lib().dpe_host_edge_segment_connect(*args, None, None, 0, C.byref(ow), C.byref(oh)) != 0:
        raise PipelineError("EdgeSegment failed")
    lab = np.empty((oh.value, ow.value), np.int32)
    bgr = np.empty((oh.value, ow.value, 3), np.uint8)
    if lib().dpe_host_edge_segment_connect(*args, lab.ctypes.data, bgr.ctypes.data, lab.size, C.byref(ow), C.byref(oh)) != 0:
        raise PipelineError("EdgeSegment failed")
    return lab, bgr


def canny(img: np.ndarray, low: float, high: float) -> np.ndarray:
    """cv::Canny(img, low, high, 3, L2gradient=true) -> uint8 0/255."""
    a = _u8(img)
    out = np.empty_like(a)
    lib().dpe_host_canny(a.ctypes.data, a.shape[1], a.shape[0], low, high, out.ctypes.data)
    return out


def resize_u8(img: np.ndarray, new_w: int, new_h: int) -> np.ndarray:
    """cv::resize(INTER_LINEAR) of an 8-bit image."""
    a = _u8(img)
    out = np.empty((new_h, new_w), np.uint8)
    lib().dpe_host_resize_u8(a.ctypes.data, a.shape[1], a.shape[0], out.ctypes.data, new_w, new_h)
    return out


def connect(img: np.ndarray):
    """Connect (DPE.cpp:27-127) -> (labels int32, counts per label)."""
    a = _u8(img)
    lab = np.empty(a.shape, np.int32)
    n = lib().dpe_host_connect(a.ctypes.data, a.shape[1], a.shape[0], lab.ctypes.data, None, 0)
    cnt = np.empty(max(n, 1), np.int32)
    lib().dpe_host_connect(a.ctypes.data, a.shape[1], a.shape[0], lab.ctypes.data, cnt.ctypes.data, n)
    return lab, cnt[:n]


def hough_lines_p(img: np.ndarray, rho: float, theta: float, threshold: int, min_len: float, max_gap: float) -> np.ndarray:
    """cv::HoughLinesP -> int32 [n, 4] segments (x0, y0, x1, y1)."""
    a = _u8(img)
    n = lib().dpe_host_hough_lines_p(a.ctypes.data, a.shape[1], a.shape[0], rho, theta, threshold, min_len, max_gap, None, 0)
    out = np.empty((max(n, 0), 4), np.int32)
    if n > 0:
        lib().dpe_host_hough_lines_p(a.ctypes.data, a.shape[1], a.shape[0], rho, theta, threshold, min_len, max_gap,
                                     out.ctypes.data, n)
    return out


# ------------------------------------------------------------------------------ dataset writers
CV_8UC1, CV_8SC1, CV_32SC1, CV_32FC1, CV_32FC3 = 0, 1, 4, 5, 21
_CV = {CV_8UC1: (np.uint8, 1), CV_8SC1: (np.int8, 1), CV_32SC1: (np.int32, 1), CV_32FC1: (np.float32, 1),
       CV_32FC3: (np.float32, 3)}


def read_bin_mat(path: str) -> np.ndarray:
    """ReadBinMat (DPE.cpp:293-318)."""
    with open(path, "rb") as f:
        version, rows, cols, typ = struct.unpack("<4i", f.read(16))
        if version != 1 or typ not in _CV:
            raise PipelineError(f"bad .dmb: {path}")
        dt, ch = _CV[typ]
        a = np.frombuffer(f.read(), dtype=dt)[: rows * cols * ch]
    return a.reshape((rows, cols, ch) if ch > 1 else (rows, cols)).copy()


def write_bin_mat(path: str, mat: np.ndarray) -> None:
    """WriteBinMat (DPE.cpp:320-339)."""
    mat = np.ascontiguousarray(mat)
    ch = mat.shape[2] if mat.ndim == 3 else 1
    typ = {("uint8", 1): CV_8UC1, ("int8", 1): CV_8SC1, ("int32", 1): CV_32SC1, ("uint32", 1): CV_32SC1,
           ("float32", 1): CV_32FC1, ("float32", 3): CV_32FC3}[(mat.dtype.name, ch)]
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", 1, mat.shape[0], mat.shape[1], typ))
        f.write(mat.tobytes())


def write_camera(path: str, K, R, t, dmin: float, dmax: float, depth_num: int = 192) -> None:
    """cams/%08d_cam.txt as ReadCamera parses it (4-number depth line)."""
    g = lambda v: repr(float(v))  # noqa: E731
    with open(path, "w") as f:
        f.write("extrinsic\n")
        for i in range(3):
            f.write(f"{g(R[i][0])} {g(R[i][1])} {g(R[i][2])} {g(t[i])}\n")
        f.write("0.0 0.0 0.0 1.0\n\nintrinsic\n")
        for i in range(3):
            f.write(f"{g(K[i][0])} {g(K[i][1])} {g(K[i][2])}\n")
        f.write(f"\n{g(dmin)} {g((dmax - dmin) / depth_num)} {depth_num} {g(dmax)}\n")


def std_round(v) -> int:
    """std::round (half away from zero) of a non-negative value."""
    f = math.floor(float(v))
    return int(f + 1) if float(v) - f >= 0.5 else int(f)


# ------------------------------------------------------------------------------ the pipeline
def _torch_allgather(dist):
    import torch
    world = dist.get_world_size()
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")

    def cb(_user, send, count, recv):
        try:
            s = torch.from_numpy(np.ctypeslib.as_array(send, shape=(count,)).copy()).to(dev)
            out = torch.empty(world * count, dtype=torch.float32, device=dev)
            dist.all_gather_into_tensor(out, s)
            np.ctypeslib.as_array(recv, shape=(world * count,))[:] = out.cpu().numpy()
            return 0
        except Exception:   # noqa: BLE001 -- reported to the C++ side as a failed collective
            return -1
    return ALLGATHER_FN(cb)


ALLGATHER_DEV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class _DeviceArray:
    """A device buffer of the library as a torch tensor view (__cuda_array_interface__, no copy)."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 3}


def _torch_allgather_device(dist):
    """Device all-gather hook (dpe_allgather_dev_fn) over torch.distributed "nccl" (= RCCL): the
    depth maps go from the library's HBM buffers to the other ranks' without a host copy."""
    import torch
    world = dist.get_world_size()

    def cb(_user, send, count, recv):
        try:
            s = torch.as_tensor(_DeviceArray(send, count), device="cuda")
            r = torch.as_tensor(_DeviceArray(recv, world * count), device="cuda")
            dist.all_gather_into_tensor(r, s)
            torch.cuda.synchronize()
            return 0
        except Exception:   # noqa: BLE001 -- reported to the C++ side as a failed collective
            return -1
    return ALLGATHER_DEV_FN(cb)


def run_dpe_pipeline(dense_folder: str, gpu_index: int = 0, verbose: bool = True, fusion: bool = False,
                     viz: bool = False, depth: bool = True, normal: bool = False, weak: bool = False,
                     edge: bool = False, schedule: str = "reference", dist=None, runner=None,
                     base_seed: int = 0x5EED, keep_intermediate: bool = False, fusion_runner=None,
                     max_iterations: int = 0, photometric_only: bool = False, allgather_device=None,
                     fusion_mode="eth3d", point_cloud=0, consistency: int = 0) -> int:
    """RunDPEPipeline (main.cpp:474) through libdpe_host.  `dist`: an initialised torch.distributed
    (one process per GPU; problems split in contiguous blocks, depth maps all-gathered per pass).
    `runner`: (C function pointer, user pointer) of a dpe_pass_runner_fn; default the HIP library.
    `fusion_runner`: (C function pointer, user pointer) of a dpe_fusion_fn; default the HIP kernel.
    `max_iterations` (0 = the reference's 3) and `photometric_only` (no geometric passes) are the
    schedule knobs of BASELINE configs 1 and 2.  `allgather_device`: a Python callable
    (send_ptr, count, recv_ptr) -> int used as the device all-gather hook instead of the torch "nccl"
    one (tests drive the device exchange path through it on one GPU).  `fusion_mode`: "eth3d"
    (RunFusion, the default), "tat_intermediate" or "tat_advanced" (the Tanks-and-Temples fusions, one
    image at a time on the GPU; with a `fusion_runner` their serial loops on the host), or the integer
    of DpePipelineOptions.fusion_mode.  `point_cloud`: 0 / "off" (the default), 1 / "all" or 2 / "strong":
    every reference image's point_<it>.ply (ExportDepthImagePointCloud) after the last pass of every
    resolution round; "strong" keeps the STRONG pixels only (main.cpp:464).  `consistency`: 0 (the default)
    off, or min_views 1..255: every reference image's consistency.npy (u8 [H, W]: the source views that pass
    RunFusion's reprojection, depth and angle tests at the pixel, without its masks and blocks) and
    depth_filtered.npy (f32 [H, W]: the final depth where that count >= min_views, else 0); on the GPU, or
    with a `fusion_runner` on host threads; any other value raises PipelineError."""
    o = DpePipelineOptions()
    lib().dpe_pipeline_default_options(C.byref(o))
    o.fusion_mode = _fusion_mode(fusion_mode)
    o.point_cloud = _point_cloud_mode(point_cloud)
    o.consistency = int(consistency)
    o.gpu_index = gpu_index
    o.verbose, o.fusion, o.viz, o.depth, o.normal, o.weak, o.edge = verbose, fusion, viz, depth, normal, weak, edge
    o.schedule = {"reference": SCHEDULE_REFERENCE, "jacobi": SCHEDULE_JACOBI}[schedule]
    o.base_seed = base_seed
    o.keep_intermediate = keep_intermediate
    o.max_iterations = max_iterations
    o.photometric_only = photometric_only
    keep = []
    if dist is not None and dist.get_world_size() > 1:
        o.rank, o.world_size = dist.get_rank(), dist.get_world_size()
        cb = _torch_allgather(dist)
        keep.append(cb)
        o.allgather = cb
        if allgather_device is not None:
            dcb = ALLGATHER_DEV_FN(lambda _user, send, count, recv: int(allgather_device(send, count, recv)))
            keep.append(dcb)
            o.allgather_device = C.cast(dcb, C.c_void_p)
        elif dist.get_backend() == "nccl" and runner is None:
            dcb = _torch_allgather_device(dist)
            keep.append(dcb)
            o.allgather_device = C.cast(dcb, C.c_void_p)
    if runner is not None:
        o.runner = C.cast(runner[0], C.c_void_p)
        o.runner_user = C.cast(runner[1], C.c_void_p) if runner[1] is not None else None
    if fusion_runner is not None:
        o.fusion_runner = C.cast(fusion_runner[0], C.c_void_p)
        o.fusion_user = C.cast(fusion_runner[1], C.c_void_p) if fusion_runner[1] is not None else None
    rc = lib().dpe_run_pipeline(dense_folder.encode(), C.byref(o))
    if rc != 0:
        raise PipelineError(lib().dpe_pipeline_last_error().decode(errors="replace"))
    return rc


def dpe_mvs(dense_folder: str, gpu_index: int = 0, verbose: bool = True, fusion: bool = False, viz: bool = False,
            depth: bool = True, normal: bool = False, weak: bool = False, edge: bool = False, *,
            fusion_mode: str = "eth3d") -> int:
    """DPE_MVS.dpe_mvs through the pybind11 module (csrc/bindings.cpp:31-43 equivalent)."""
    from ._dpe import dpe_mvs as _native
    return _native(dense_folder, gpu_index, verbose, fusion, viz, depth, normal, weak, edge, fusion_mode=fusion_mode)
