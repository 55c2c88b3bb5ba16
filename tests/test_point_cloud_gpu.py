"""Per-image point clouds on the device (csrc/pass_points.h, dpe_state_point_cloud / dpe_point_cloud_arrays
of include/dpe_mvs.h): the kernels must give the host loop's points bit for bit and in its column-major
order (the host loop is checked against numpy in tests/test_point_cloud.py), the resident pipeline must
write the host path's files, and a run without the option must launch none of the new kernels."""
import ctypes as C
import os

import numpy as np
import pytest

from DPE_MVS import _abi, native, pipeline, synthetic
from test_pipeline import _copy
from test_point_cloud import (DMAX, DMIN, F, adversarial_depth, bits, check_point_cloud_run, cloud_camera, every_state_weak,
                              files_under, random_bgr, recording_runner)

pytestmark = pytest.mark.gpu
SEG, COLS = 32, 256          # kPtsSeg, kPtsCols of csrc/pass_points.h: rows per cell, columns per block


@pytest.fixture(scope="module")
def ctx():
    c = native.PatchMatchContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------ 5. device vs host on a real state
@pytest.mark.parametrize("W,H", [(64, 48), (50, 33)])
def test_state_point_cloud_matches_host(ctx, W, H):
    """The one-iteration pass of test_viz_gpu.py::test_state_render_matches_host + dpe_state_save: a real
    post-epilogue state with all three pixel states."""
    sc = synthetic.make_scene(W, H, 4)
    p = _abi.default_params()
    p.state = _abi.REFINE_ITER
    p.geom_consistency = True
    p.rotate_time = 2
    p.ransac_threshold = 0.00875
    p.max_scale_size = 2
    p.max_iterations = 1
    inp = synthetic.pass_input(sc, p, depths=synthetic.src_depths(sc))
    st = synthetic.gt_state(sc)
    st["planes"] = st["planes"].copy()
    st["planes"][5:9, 7:20, 3] = np.float32(p.depth_max) * 2          # priors the pass may leave out of range
    ctx.stage(inp, st)
    ctx.execute()
    ctx.state_save(21)
    state = ctx.state_fetch(21)
    cam, bgr = sc["cams"][0], random_bgr(W, H)
    # The pass's own range, as the pipeline passes it, and one that ends at the state's median depth.  The
    # pass leaves no depth outside its range whatever the prior (finite, NaN or inf: checked with the CPU
    # oracle), so with the first every pixel is a point in mode 1; the second gives the input on which
    # 0 < n < W * H holds in both modes.
    cut = F(np.median(state["depth"]))
    n = {}
    for dmax in (F(p.depth_max), cut):
        for mode in (native.POINTS_ALL, native.POINTS_STRONG):
            got = ctx.state_point_cloud(21, mode, cam, bgr, p.depth_min, dmax)
            want = pipeline.depth_point_cloud(state["depth"], cam, bgr, p.depth_min, dmax, mode=mode, weak=state["weak"])
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (mode, dmax)
            n[(mode, dmax == cut)] = len(got)
    assert 0 < n[(native.POINTS_STRONG, False)] < n[(native.POINTS_ALL, False)] <= W * H
    assert 0 < n[(native.POINTS_STRONG, True)] < n[(native.POINTS_ALL, True)] < W * H   # (conditions on the input, not tolerances)
    n = {mode: n[(mode, False)] for mode in (native.POINTS_ALL, native.POINTS_STRONG)}
    # errors of the state entry
    with pytest.raises(native.DpeError, match=r"\(-4\).*no state"):       # DPE_ERR_STATE: unknown id
        ctx.state_point_cloud(12345, native.POINTS_ALL, cam, bgr, 0, 1)
    with pytest.raises(native.DpeError, match=r"\(-1\).*bad mode"):       # DPE_ERR_ARG
        ctx.state_point_cloud(21, 3, cam, bgr, p.depth_min, p.depth_max)
    with pytest.raises(native.DpeError, match=r"\(-1\).*too small"):      # DPE_ERR_ARG: cap one short
        ctx.state_point_cloud(21, native.POINTS_ALL, cam, bgr, p.depth_min, p.depth_max, cap=n[native.POINTS_ALL] - 1)
    assert len(ctx.state_point_cloud(21, native.POINTS_ALL, cam, bgr, p.depth_min, p.depth_max, cap=n[native.POINTS_ALL])) == \
        n[native.POINTS_ALL]


def test_depth_only_state(ctx):
    """A state imported from another rank holds a depth map only: fine in mode 1, DPE_ERR_STATE in mode 2."""
    w, h = 37, 35
    depth, kept = adversarial_depth(w, h)
    cam, bgr = cloud_camera(w, h), random_bgr(w, h)
    ctx.state_import_depth(31, depth)
    got = ctx.state_point_cloud(31, native.POINTS_ALL, cam, bgr, DMIN, DMAX)
    assert len(got) == kept and np.array_equal(bits(got), bits(pipeline.depth_point_cloud(depth, cam, bgr, DMIN, DMAX)))
    with pytest.raises(native.DpeError, match=r"\(-4\).*depth map only"):
        ctx.state_point_cloud(31, native.POINTS_STRONG, cam, bgr, DMIN, DMAX)


# ------------------------------------------------------------------------------ 6. the scan's shapes
def in_range(w, h, seed=2):
    return np.random.default_rng(seed).uniform(3.0, 8.0, (h, w)).astype(np.float32)


def case_checkerboard(w, h):
    d = in_range(w, h)
    d[(np.add.outer(np.arange(h), np.arange(w)) % 2) == 1] = F(0)
    return d


def case_ragged(w, h):
    """Runs of valid and invalid pixels of changing length down the columns, different in every column."""
    d = in_range(w, h)
    j, i = np.mgrid[0:h, 0:w]
    d[((j * 7 + i * 13) % 11) < 4] = F(np.nan)
    d[((j * 3 + i * 5) % 17) == 0] = F(100.0)
    return d


SHAPES = [
    ("one_pixel", 1, 1, in_range),
    ("column_one_taller_than_a_segment", 1, SEG + 1, in_range),
    ("one_more_column_than_a_block", COLS + 1, 3, case_ragged),
    ("off_the_tile_both_ways", COLS + 44, 2 * SEG + 6, case_ragged),
    ("all_valid", 33, SEG + SEG + 1, in_range),
    ("checkerboard", 70, 45, case_checkerboard),
    ("adversarial_7x5", 7, 5, lambda w, h: adversarial_depth(w, h)[0]),
    ("adversarial_5x7", 5, 7, lambda w, h: adversarial_depth(w, h)[0]),
]


@pytest.mark.parametrize("name,w,h,make", SHAPES, ids=[s[0] for s in SHAPES])
def test_point_cloud_arrays_match_host(ctx, name, w, h, make):
    depth = make(w, h)
    cam, bgr, weak = cloud_camera(w, h), random_bgr(w, h), every_state_weak(w, h)
    for mode, dmin in ((1, DMIN), (2, DMIN), (2, F(0))):              # dmin = 0: mode 2 replaces, it does not drop
        want = pipeline.depth_point_cloud(depth, cam, bgr, dmin, DMAX, mode=mode, weak=weak)
        got = ctx.point_cloud_arrays(mode, depth, cam, bgr, dmin, DMAX, weak=weak, cap=len(want))   # cap exact
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (mode, dmin)
    full = pipeline.depth_point_cloud(depth, cam, bgr, DMIN, DMAX)
    assert np.array_equal(bits(ctx.point_cloud_arrays(1, depth, cam, bgr, DMIN, DMAX)), bits(full))   # weak = None
    if name == "all_valid":
        assert len(full) == w * h
    if len(full):
        with pytest.raises(native.DpeError, match=r"\(-1\).*too small"):
            ctx.point_cloud_arrays(1, depth, cam, bgr, DMIN, DMAX, cap=len(full) - 1)


def test_point_cloud_arrays_all_invalid_and_errors(ctx):
    w, h = 40, 40
    cam, bgr = cloud_camera(w, h), random_bgr(w, h)
    depth = np.full((h, w), np.nan, np.float32)
    depth[::2] = F(0)
    before = native.points_launches()
    assert ctx.point_cloud_arrays(1, depth, cam, bgr, DMIN, DMAX).shape == (0, 6)
    assert native.points_launches() == before + 3                     # count, offsets, fill
    assert ctx.point_cloud_arrays(1, depth, cam, bgr, DMIN, DMAX, cap=0).shape == (0, 6)   # nothing written, no copy
    with pytest.raises(native.DpeError, match=r"\(-1\).*bad mode"):
        ctx.point_cloud_arrays(0, depth, cam, bgr, DMIN, DMAX)
    with pytest.raises(native.DpeError, match=r"\(-1\).*missing array"):   # mode 2 needs the states
        ctx.point_cloud_arrays(2, depth, cam, bgr, DMIN, DMAX)


# ------------------------------------------------------------------------------ 7. resident pipeline
@pytest.fixture(scope="module")
def dense4(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pointsgpu"))
    synthetic.write_dense_folder(d, 64, 48, 4)
    return d


def test_resident_pipeline_writes_the_host_paths_files(tmp_path, dense4, ctx):
    """The default (resident) runner against a runner-hook run whose runner is the HIP library's dpe_pm_run:
    the same passes, the state on the device there and on the host here, the same point_<it>.ply files."""
    a = _copy(dense4, tmp_path, "resident")
    b = _copy(dense4, tmp_path, "hook")
    launches, live = native.points_launches(), native.live_device_bytes()
    assert pipeline.run_dpe_pipeline(a, normal=True, weak=True, verbose=False, point_cloud=1) == 0
    assert native.points_launches() == launches + 4 * 2 * 3            # 4 images, 2 rounds, 3 kernels
    assert native.live_device_bytes() == live                          # the run's context gave everything back
    states, ranges = {}, {}
    hip_runner = (C.cast(native._LIB.dpe_pm_run, C.c_void_p), ctx._ctx)
    keep, runner = recording_runner(b, hip_runner, states, ranges)
    assert pipeline.run_dpe_pipeline(b, runner=runner, normal=True, weak=True, verbose=False, keep_intermediate=True,
                                     point_cloud=1) == 0
    check_point_cloud_run(tmp_path, b, states, ranges, 1)              # the hook run's files are its states' clouds
    fa, fb = files_under(a), files_under(b)
    names = sorted(f for f in fa if "point_" in f)
    assert len(names) == 8 and names == sorted(f for f in fb if "point_" in f)
    for f in names + [os.path.join("DPE", f"{i:08d}", o) for i in range(4) for o in ("depth.npy", "normal.npy", "weak.npy")]:
        assert fa[f] == fb[f], f
    del keep


def test_point_cloud_off_launches_nothing(tmp_path, dense4):
    a = _copy(dense4, tmp_path, "off")
    launches, live = native.points_launches(), native.live_device_bytes()
    assert pipeline.run_dpe_pipeline(a, normal=True, weak=True, verbose=False, point_cloud=0) == 0
    assert native.points_launches() == launches and native.live_device_bytes() == live
    assert not [f for f in files_under(a) if "point_" in f]
