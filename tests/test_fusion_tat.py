"""The two Tanks-and-Temples fusions, RunFusion_TAT_Intermediate (DPE.cpp:1372-1540) and
RunFusion_TAT_advanced (DPE.cpp:1542-1689), behind `fusion_mode`.

The yardstick is the reference's serial loop restated in host/fusion_tat.cpp (dpe_host_fusion_tat_serial),
stale per-view `diff` entries included; the known-answer tests below pin that loop with expected values
worked out by hand, and everything else (the device path of dpe_fusion_tat_image, the pipeline) is
compared with it bit for bit.

The pipeline tests run on an 80x60, 4-view synthetic folder: at 64x48 with 4 views the strict k = 2
thresholds (0.5 px, 1/1750) leave the yardstick 20 (Intermediate) and 79 (Advanced) points, at 80x60
it gives 165 and 311, which clears the bar of 100."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import oracle
from DPE_MVS import _abi, pipeline, synthetic
from test_fusion import _final_views, _free_port, oracle_runner, read_ply

MODES = ["tat_intermediate", "tat_advanced"]
PW, PH, PV = 80, 60, 4     # the pipeline tests' folder (see the module docstring)


# ------------------------------------------------------------------------------ hand-built scenes
def plane_scene(W, H, hole=False, seed=7, hole_rows=(10, 31)):
    """Three identical cameras (fx = 64, principal point (32, 24), R = I, t = 0) looking at the plane
    z = 4: every value below is exact in float32, so pixel p of any view projects onto pixel p of any
    other with reprojection error 0, depth difference 0 and normal dot product 1.  `hole`: the two
    later views have no depth over rows 10-30 (`hole_rows`, end exclusive)."""
    rng = np.random.default_rng(seed)
    cam = _abi.DpeCamera()
    K = [64.0, 0.0, 32.0, 0.0, 64.0, 24.0, 0.0, 0.0, 1.0]
    R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for i in range(9):
        cam.K[i], cam.R[i] = K[i], R[i]
    cam.width, cam.height, cam.depth_min, cam.depth_max = W, H, 1.0, 10.0
    views = []
    for i in range(3):
        depth = np.full((H, W), 4.0, np.float32)
        if hole and i > 0:
            depth[hole_rows[0]:hole_rows[1]] = 0.0
        normal = np.zeros((H, W, 3), np.float32)
        normal[..., 2] = -1.0
        views.append(dict(image_id=i, src_ids=[j for j in range(3) if j != i], cam=cam, depth=depth, normal=normal,
                          bgr=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), block=None))
    return views


def plane_points(W, H):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    four = np.float32(4.0)
    return np.stack([four * (xx - np.float32(32)) / np.float32(64), four * (yy - np.float32(24)) / np.float32(64),
                     np.full((H, W), four)], -1).reshape(-1, 3)


def expected_plane(views, mode, hole):
    """Image 0 fuses every pixel with both sources; images 1 and 2 then find view 0 masked and are left
    with one view, count = 1 < 2.  In the hole the sources do not hit, and the entries of the last
    pixel before it, (row 9, last column), are still in `diff`: dist 0, depth 0, angle 0."""
    H, W = views[0]["depth"].shape
    col = views[0]["bgr"].reshape(-1, 3).astype(np.float32)
    if mode == "tat_intermediate":
        src = [v["bgr"].astype(np.float32).copy() for v in views[1:]]
        if hole:
            for s in src:
                s[10:31] = s[9, W - 1]
        col = ((col + src[0].reshape(-1, 3)) + src[1].reshape(-1, 3)) / np.float32(3.0)
    return plane_points(W, H), col


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hole", [False, True])
def test_serial_known_answers_on_three_identical_cameras(mode, hole):
    views = plane_scene(64, 48, hole)
    pts, masks = pipeline.fusion_tat_serial(views, mode)
    xyz, col = expected_plane(views, mode, hole)
    assert len(pts) == 3072                      # image 0: all pixels (the hole's 1344 through the stale entries)
    assert masks[0].all() and not masks[1].any() and not masks[2].any()
    assert np.array_equal(pts[:, :3].view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(pts[:, 3:].view(np.uint32), col.view(np.uint32))
    if hole and mode == "tat_intermediate":      # the carried source pixel, not the one under the hole
        fresh = (views[0]["bgr"].astype(np.float32) + views[1]["bgr"] + views[2]["bgr"]) / np.float32(3.0)
        assert not np.array_equal(pts[10 * 64:31 * 64, 3:], fresh[10:31].reshape(-1, 3))


def test_serial_without_the_stale_entries_would_drop_the_hole():
    """The same hole as seen by image 2 first: no pixel before the hole is lost, and a reference image
    whose FIRST rows miss their sources has no entry to carry, so those rows are not fused."""
    views = plane_scene(64, 48)
    for v in views[1:]:
        v["depth"][0:5] = 0.0
    pts, masks = pipeline.fusion_tat_serial(views, "tat_advanced")
    assert len(pts) == 3072 - 5 * 64 and not masks[0][:5].any() and masks[0][5:].all()


@pytest.mark.parametrize("mode", MODES)
def test_one_source_view_gives_no_points(mode, tmp_path):
    views = plane_scene(64, 48)[:2]
    views[0]["src_ids"], views[1]["src_ids"] = [1], [0]
    pts, masks = pipeline.fusion_tat_serial(views, mode)
    assert len(pts) == 0 and not masks[0].any() and not masks[1].any()
    d = str(tmp_path / "two")
    synthetic.write_dense_folder(d, 64, 48, 2)                      # every image has one source: ns = 1
    assert pipeline.run_dpe_pipeline(d, runner=oracle_runner(), fusion_runner=oracle.fusion_runner(), fusion=True,
                                     verbose=False, fusion_mode=mode) == 0
    xyz, _ = read_ply(os.path.join(d, "DPE", "DPE.ply"))
    assert len(xyz) == 0


# ------------------------------------------------------------------------------ threshold table
def test_threshold_table_agrees_with_getangle_around_every_threshold():
    D = pipeline.fusion_tat_thresholds(32)
    assert D.dtype == np.float32 and len(D) == 32
    assert np.all(np.diff(D[2:]) < 0) and np.all(D[2:] > -1) and np.all(D[2:] < 1)
    test = pipeline.lib().dpe_host_fusion_tat_angle_test
    for k in range(2, 32):
        bits = int(D[k:k + 1].view(np.int32)[0])
        # the 4096 floats on each side: for a positive float the next one up is bits + 1, for a negative one bits - 1
        step = 1 if D[k] > 0 else -1
        assert abs(D[k]) > 1e-3                  # no neighbour crosses zero, where the bit order flips
        near = (bits + step * np.arange(-4096, 4097)).astype(np.int32).view(np.float32)
        assert np.all(np.diff(near) > 0) and near[4096] == D[k]
        got = np.array([test(float(x), k) for x in near], bool)
        assert np.array_equal(got, near >= D[k]), k


# ------------------------------------------------------------------------------ pipeline (CPU: oracle passes, serial fusion)
def _run(d, mode, **kw):
    return pipeline.run_dpe_pipeline(d, runner=oracle_runner(), fusion_runner=oracle.fusion_runner(), fusion=True,
                                     verbose=False, keep_intermediate=True, fusion_mode=mode, **kw)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """One dense folder per mode, fused by the CPU pipeline (oracle passes, the serial fusion)."""
    out = {}
    first = None
    for mode in MODES:
        d = str(tmp_path_factory.mktemp(mode))
        if first is None:
            synthetic.write_dense_folder(d, PW, PH, PV)
            first = d
        else:
            shutil.rmtree(d)
            shutil.copytree(first, d)
        out[mode] = d
    for mode, d in out.items():
        assert _run(d, mode) == 0
    return out


def _ply(d):
    return open(os.path.join(d, "DPE", "DPE.ply"), "rb").read()


def _assert_ply_is_serial(d, mode, views):
    xyz, bgr = read_ply(os.path.join(d, "DPE", "DPE.ply"))
    ref, _ = pipeline.fusion_tat_serial(views, mode)
    assert ref.shape[0] == xyz.shape[0]
    assert np.array_equal(ref[:, :3].view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(ref[:, 3:].astype(np.uint8), bgr)                        # static_cast<uchar>
    return len(xyz)


@pytest.mark.parametrize("mode", MODES)
def test_pipeline_ply_equals_serial_yardstick(folders, mode):
    views = _final_views(folders[mode], PV)
    n = _assert_ply_is_serial(folders[mode], mode, views)
    assert n > 100
    # not the default mode's cloud: RunFusion over the same maps (what the default mode writes from them,
    # test_fusion.py) keeps other points
    default = oracle.run_fusion(views)
    assert default.shape[0] > 100 and default.shape[0] != n
    assert _ply(folders["tat_intermediate"]) != _ply(folders["tat_advanced"])


def test_pipeline_with_block_masks_matches_yardstick(tmp_path, folders):
    from PIL import Image
    d = str(tmp_path / "blk")
    synthetic.write_dense_folder(d, PW, PH, PV)
    os.makedirs(os.path.join(d, "blocks"))
    for i in range(PV):
        m = np.zeros((PH, PW), np.uint8)
        m[:, 10 + 4 * i:] = 255
        Image.fromarray(m, mode="L").save(os.path.join(d, "blocks", f"mask_{i}.jpg"), quality=95)
    assert _run(d, "tat_advanced") == 0
    views = _final_views(d, PV)
    for i, v in enumerate(views):
        v["block"] = pipeline.read_gray(os.path.join(d, "blocks", f"mask_{i}.jpg"))
    n = _assert_ply_is_serial(d, "tat_advanced", views)
    assert 0 < n and _ply(d) != _ply(folders["tat_advanced"])


def _rank_main(rank, world, port, folder, mode):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        assert pipeline.run_dpe_pipeline(folder, runner=oracle_runner(), fusion_runner=oracle.fusion_runner(),
                                         fusion=True, verbose=False, dist=dist, fusion_mode=mode) == 0
    finally:
        dist.destroy_process_group()


def test_two_rank_run_matches_one_rank(tmp_path):
    import torch.multiprocessing as mp
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    synthetic.write_dense_folder(one, 64, 48, 4)
    shutil.copytree(one, two)
    assert pipeline.run_dpe_pipeline(one, runner=oracle_runner(), fusion_runner=oracle.fusion_runner(), fusion=True,
                                     schedule="jacobi", verbose=False, fusion_mode="tat_advanced") == 0
    mp.start_processes(_rank_main, args=(2, _free_port(), two, "tat_advanced"), nprocs=2, join=True, start_method="spawn")
    a, b = _ply(one), _ply(two)
    assert a == b and len(read_ply(os.path.join(one, "DPE", "DPE.ply"))[0]) > 0


def test_invalid_fusion_mode_fails_with_a_message(tmp_path):
    d = str(tmp_path / "bad")
    synthetic.write_dense_folder(d, 64, 48, 3)
    with pytest.raises(pipeline.PipelineError, match="fusion_mode"):
        pipeline.run_dpe_pipeline(d, runner=oracle_runner(), verbose=False, fusion_mode=7)
    with pytest.raises(ValueError, match="fusion_mode"):
        pipeline.run_dpe_pipeline(d, runner=oracle_runner(), verbose=False, fusion_mode="tanks")
    o = pipeline.DpePipelineOptions()
    pipeline.lib().dpe_pipeline_default_options(C.byref(o))
    assert o.fusion_mode == pipeline.FUSION_ETH3D
    o.fusion_mode = -1
    assert pipeline.lib().dpe_run_pipeline(d.encode(), C.byref(o)) != 0
    assert b"fusion_mode" in pipeline.lib().dpe_pipeline_last_error()


def test_dpe_mvs_keeps_the_nine_reference_arguments():
    """fusion_mode is a trailing keyword of the pybind entry: the reference's nine arguments keep their
    positions and defaults (the GPU test below runs them)."""
    import inspect
    import DPE_MVS
    from DPE_MVS import _dpe
    args = _dpe.dpe_mvs.__doc__.split("dpe_mvs(", 1)[1].split(") -> int", 1)[0].split(", ")
    assert [a.split(":")[0] for a in args] == ["dense_folder", "gpu_index", "verbose", "fusion", "viz", "depth", "normal",
                                               "weak", "edge", "*", "fusion_mode"]
    assert [a.rsplit("= ", 1)[-1] for a in args[1:9]] == ["0", "True", "False", "False", "True", "False", "False", "False"]
    assert args[-1] == "fusion_mode: str = 'eth3d'"
    p = inspect.signature(DPE_MVS.dpe_mvs).parameters
    assert list(p) == ["dense_folder", "gpu_index", "verbose", "fusion", "viz", "depth", "normal", "weak", "edge", "fusion_mode"]
    assert p["fusion_mode"].kind is inspect.Parameter.KEYWORD_ONLY and p["fusion_mode"].default == "eth3d"
    with pytest.raises(ValueError, match="fusion_mode"):
        _dpe.dpe_mvs("/nonexistent", fusion_mode="tanks")
    with pytest.raises(TypeError):
        _dpe.dpe_mvs("/nonexistent", 0, True, False, False, True, False, False, False, "tat_advanced")


# ------------------------------------------------------------------------------ GPU
def _device_fuse(lib, ctx, views, mode):
    """dpe_fusion_stage + dpe_fusion_tat_begin + one dpe_fusion_tat_image per view, in order."""
    from DPE_MVS import native
    arr, keep = native.fusion_view_array([(v["depth"], v["normal"], v["cam"]) for v in views])
    n = len(views)
    bgr = [np.ascontiguousarray(v["bgr"], np.uint8) for v in views]
    blk = [None if v["block"] is None else np.ascontiguousarray(v["block"], np.uint8) for v in views]
    pb = (C.c_void_p * n)(*[a.ctypes.data for a in bgr])
    pk = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in blk])
    D = pipeline.fusion_tat_thresholds(32)
    assert lib.dpe_fusion_stage(ctx, arr, n) == 0
    assert lib.dpe_fusion_tat_begin(ctx, pb, pk) == 0, lib.dpe_last_error()
    index = {v["image_id"]: i for i, v in enumerate(views)}
    clouds = []
    for i, v in enumerate(views):
        src = np.array([index[s] for s in v["src_ids"]], np.int32)
        out = np.empty((v["depth"].size, 6), np.float32)
        cnt = C.c_size_t()
        assert lib.dpe_fusion_tat_image(ctx, pipeline.FUSION_MODES[mode], i, src.ctypes.data, len(src), D.ctypes.data,
                                        out.ctypes.data, len(out), C.byref(cnt)) == 0, lib.dpe_last_error()
        clouds.append((out, cnt.value))
    assert lib.dpe_fusion_tat_wait(ctx) == 0
    masks = []
    for i, v in enumerate(views):
        m = np.empty(v["depth"].shape, np.uint8)
        assert lib.dpe_fusion_tat_mask(ctx, i, m.ctypes.data) == 0
        masks.append(m)
    return np.concatenate([o[:c] for o, c in clouds]), masks


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size,hole", [((64, 48), False), ((64, 48), True), ((61, 47), False), ((61, 47), True)])
def test_gpu_tat_image_matches_yardstick_on_hand_built_scenes(mode, size, hole):
    from DPE_MVS import native
    lib = native.load_library()
    views = plane_scene(size[0], size[1], hole)
    ref, ref_masks = pipeline.fusion_tat_serial(views, mode)
    assert len(ref) == size[0] * size[1]
    before = native.live_device_bytes()
    ctx = lib.dpe_create(0)
    try:
        pts, masks = _device_fuse(lib, ctx, views, mode)
        assert native.live_device_bytes() > before
    finally:
        lib.dpe_destroy(ctx)
    assert native.live_device_bytes() == before
    assert pts.shape == ref.shape and np.array_equal(pts.view(np.uint32), ref.view(np.uint32))   # points, colours, order
    for a, b in zip(masks, ref_masks):
        assert np.array_equal(a, b)


def ragged_block(W, H):
    """A block mask that drops the pixels with (x * 7 + y * 13) % 5 == 0 and the whole of rows 60 to 139."""
    yy, xx = np.mgrid[0:H, 0:W]
    keep = (xx * 7 + yy * 13) % 5 != 0
    keep[60:140] = False
    return np.where(keep, 255, 0).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [(331, 199), (7, 5)])
def test_gpu_tat_image_matches_yardstick_with_unequal_chunk_counts(mode, size):
    """The chunk counts and their offsets where they differ from chunk to chunk: every view carries ragged_block, so
    image 0 fuses exactly the pixels it keeps and a chunk holds anything from 0 to 206 points.  331x199 = 65,869
    pixels = 258 chunks, the last with 77 pixels: unequal counts on both sides of the 256-chunk tile of the offsets
    scan (chunks 256 and 257 hold 205 and 62 points) and a run of 103 empty chunks (rows 60 to 139).
    7x5 = 35 pixels: one chunk with less than one wave."""
    from DPE_MVS import native
    lib = native.load_library()
    W, H = size
    views = plane_scene(W, H)
    for v in views:
        v["block"] = ragged_block(W, H)
    ref, ref_masks = pipeline.fusion_tat_serial(views, mode)
    assert 0 < len(ref) < W * H                      # the comparison below is not over nothing, nor over every pixel
    assert np.array_equal(ref_masks[0] == 1, views[0]["block"] >= 128)
    ctx = lib.dpe_create(0)
    try:
        pts, masks = _device_fuse(lib, ctx, views, mode)
    finally:
        lib.dpe_destroy(ctx)
    assert pts.shape == ref.shape and np.array_equal(pts.view(np.uint32), ref.view(np.uint32))   # points, colours, order
    for a, b in zip(masks, ref_masks):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_carry_crosses_more_chunks_than_one_scan_tile(mode):
    """320x208 = 260 chunks of 256 pixels, more than the 256 chunks one tile of the chunk scans takes;
    the sources have depth in row 0 only, so every later pixel is fused through the entries of pixel
    (0, 319), carried over 259 chunks and across the tile boundary."""
    from DPE_MVS import native
    lib = native.load_library()
    W, H = 320, 208
    views = plane_scene(W, H, True, hole_rows=(1, H))
    ref, ref_masks = pipeline.fusion_tat_serial(views, mode)
    assert len(ref) == W * H
    if mode == "tat_intermediate":
        a = views[0]["bgr"][H - 1, W - 1].astype(np.float32)
        want = ((a + views[1]["bgr"][0, W - 1]) + views[2]["bgr"][0, W - 1]) / np.float32(3.0)
        assert np.array_equal(ref[-1, 3:], want)
    ctx = lib.dpe_create(0)
    try:
        pts, masks = _device_fuse(lib, ctx, views, mode)
    finally:
        lib.dpe_destroy(ctx)
    assert pts.shape == ref.shape and np.array_equal(pts.view(np.uint32), ref.view(np.uint32))
    for a, b in zip(masks, ref_masks):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_tat_image_matches_yardstick_on_pipeline_maps(folders, mode):
    """Real maps: partial hits, stale entries of every age, views that never hit."""
    from DPE_MVS import native
    lib = native.load_library()
    views = _final_views(folders[mode], PV)
    ref, ref_masks = pipeline.fusion_tat_serial(views, mode)
    ctx = lib.dpe_create(0)
    try:
        pts, masks = _device_fuse(lib, ctx, views, mode)
    finally:
        lib.dpe_destroy(ctx)
    assert pts.shape == ref.shape and len(ref) > 100 and np.array_equal(pts.view(np.uint32), ref.view(np.uint32))
    for a, b in zip(masks, ref_masks):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_gpu_tat_image_refuses_a_reference_among_its_sources():
    from DPE_MVS import native
    lib = native.load_library()
    views = plane_scene(64, 48)
    arr, keep = native.fusion_view_array([(v["depth"], v["normal"], v["cam"]) for v in views])
    pb = (C.c_void_p * 3)(*[v["bgr"].ctypes.data for v in views])
    ctx = lib.dpe_create(0)
    try:
        out, cnt, src = np.empty((3072, 6), np.float32), C.c_size_t(), np.array([1, 0], np.int32)
        args = (ctx, pipeline.FUSION_TAT_ADVANCED, 0, src.ctypes.data, 2, None, out.ctypes.data, len(out), C.byref(cnt))
        assert lib.dpe_fusion_stage(ctx, arr, 3) == 0
        assert lib.dpe_fusion_tat_image(*args) == -4                       # DPE_ERR_STATE: no dpe_fusion_tat_begin
        assert lib.dpe_fusion_tat_begin(ctx, pb, None) == 0
        assert lib.dpe_fusion_tat_image(*args) == -1 and b"among its sources" in lib.dpe_last_error()
    finally:
        lib.dpe_destroy(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_pipeline_ply_matches_cpu(tmp_path, folders, mode):
    """The default runner (HIP passes, the fusion on the device) writes the CPU run's DPE.ply byte for
    byte.  (The nine positional arguments alone, the default fusion: test_fusion.py.)"""
    from DPE_MVS import dpe_mvs
    a = str(tmp_path / "hip")
    synthetic.write_dense_folder(a, PW, PH, PV)
    assert dpe_mvs(a, 0, False, True, False, True, False, False, False, fusion_mode=mode) == 0
    assert _ply(a) == _ply(folders[mode])
