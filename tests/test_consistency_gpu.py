"""Consistency maps on the device (csrc/pass_consistency.h, dpe_fusion_consistency of include/dpe_mvs.h): the
kernel must give the host loop's count and filtered depth bit for bit (the host loop is pinned against the
oracle and a numpy transcription in tests/test_consistency.py), the resident pipeline must write the host
path's files, and a run without the option must launch nothing of it."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from DPE_MVS import native, pipeline, synthetic
from test_consistency import adversarial_views, consistency_files, gt_views, same_bits
from test_pipeline import _copy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.PatchMatchContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def D():
    return pipeline.consistency_dot_threshold()


def check_device_is_host(ctx, D, views, ref, src, min_views):
    want_c, want_f = pipeline.consistency(views, ref, src, min_views)
    count, filtered = ctx.fusion_consistency(ref, src, D, min_views)
    assert same_bits(count, want_c) and same_bits(filtered, want_f), (ref, src, min_views)
    return count


# ------------------------------------------------------------------------------ 7. device against host
# one pixel; one pixel more than a 256-thread block, three times over; the scene of test_consistency.py
@pytest.mark.parametrize("W,H,N", [(1, 1, 2), (257, 3, 3), (67, 45, 5)])
def test_device_matches_host(ctx, D, W, H, N):
    views = gt_views(W, H, N)
    src = list(range(1, N))
    ctx.fusion_stage(views)
    for mv in (1, len(src)):
        count = check_device_is_host(ctx, D, views, 0, src, mv)
        only_c, none = ctx.fusion_consistency(0, src, D, mv, want_depth=False)      # depth_filtered = NULL
        assert none is None and same_bits(only_c, count)
        none, only_f = ctx.fusion_consistency(0, src, D, mv, want_count=False)      # count = NULL
        assert none is None and same_bits(only_f, pipeline.consistency(views, 0, src, mv)[1])
    assert count.any()
    check_device_is_host(ctx, D, views, N - 1, list(range(N - 1)), 1)               # another reference, same staging


def test_device_matches_host_with_31_sources(ctx, D):
    views = gt_views(16, 12, 32)
    ctx.fusion_stage(views)
    count = check_device_is_host(ctx, D, views, 0, list(range(1, 32)), 31)
    assert count.max() == 31 and len(np.unique(count)) > 8
    check_device_is_host(ctx, D, views, 5, [31, 0, 17], 2)


@pytest.mark.parametrize("w,h", [(7, 5), (5, 7)])
def test_device_matches_host_on_adversarial_maps(ctx, D, w, h):
    views = adversarial_views(w, h)
    ctx.fusion_stage(views)
    seen = set()
    for src in ([1, 2, 3, 4], [4, 1], [3], [2]):
        for mv in (1, len(src)):
            seen |= set(check_device_is_host(ctx, D, views, 0, src, mv).ravel().tolist())
    assert {0, 1, 2}.issubset(seen)
    assert check_device_is_host(ctx, D, views, 4, [0, 1], 1).any()                  # the other image size as the reference


# ------------------------------------------------------------------------------ 8. errors
def test_errors_and_no_sources(D):
    c = native.PatchMatchContext(0)
    try:
        with pytest.raises(native.DpeError, match=r"\(-4\).*nothing staged"):        # DPE_ERR_STATE
            c.fusion_consistency(0, [1], D, 1)
        views = gt_views(16, 12, 3)
        c.fusion_stage(views)
        for ref, src, mv, msg in ((0, [1, 2], 0, "min_views"), (0, [1, 2], 256, "min_views"), (0, [1, 3], 1, "bad source view"),
                                  (0, [-1], 1, "bad source view"), (3, [1], 1, "bad reference view"),
                                  (-1, [1], 1, "bad reference view"), (0, [1, 0], 1, "among its sources"),
                                  (0, [1, 2] * 128, 1, "more than 255")):
            with pytest.raises(native.DpeError, match=r"\(-1\).*" + msg):           # DPE_ERR_ARG
                c.fusion_consistency(ref, src, D, mv)
        s = np.array([1], np.int32)
        out = np.empty((12, 16), np.uint8)
        assert native._LIB.dpe_fusion_consistency(c._ctx, 0, s.ctypes.data, -1, D, 1, out.ctypes.data, None) == -1
        assert b"bad argument" in native._LIB.dpe_last_error()
        assert native._LIB.dpe_fusion_consistency(c._ctx, 0, None, 2, D, 1, out.ctypes.data, None) == -1
        before = native.consistency_launches()
        count, filtered = c.fusion_consistency(0, [], D, 1)                          # ns = 0: one launch, all zeros
        assert native.consistency_launches() == before + 1
        assert count.shape == (12, 16) and not count.any() and same_bits(filtered, np.zeros((12, 16), np.float32))
        count, _ = c.fusion_consistency(0, [1, 2], D, 255)                           # 255 is a valid threshold
        assert same_bits(count, pipeline.consistency(views, 0, [1, 2], 255)[0])
    finally:
        c.close()


# ------------------------------------------------------------------------------ 9. resident pipeline
@pytest.fixture(scope="module")
def dense4(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("consistencygpu"))
    synthetic.write_dense_folder(d, 64, 48, 4)
    return d


def test_resident_pipeline_writes_the_host_paths_files(tmp_path, dense4, ctx):
    """The default (resident) runner, whose maps come from dpe_fusion_consistency, against a run whose passes
    are the HIP library's dpe_pm_run through the runner hook and whose maps, a fusion_runner hook being set,
    come from dpe_host_consistency on host threads: the same files.  With fusion as well, so that RunFusion
    finds the views the filter staged."""
    a = _copy(dense4, tmp_path, "resident")
    b = _copy(dense4, tmp_path, "hook")
    launches, live = native.consistency_launches(), native.live_device_bytes()
    assert pipeline.run_dpe_pipeline(a, normal=True, weak=True, verbose=False, consistency=1, fusion=True) == 0
    assert native.consistency_launches() == launches + 4                 # one kernel per image
    assert native.live_device_bytes() == live                            # the run's context gave everything back
    hip_runner = (C.cast(native._LIB.dpe_pm_run, C.c_void_p), ctx._ctx)
    assert pipeline.run_dpe_pipeline(b, runner=hip_runner, fusion_runner=oracle.fusion_runner(), normal=True, weak=True,
                                     verbose=False, consistency=1, fusion=True) == 0
    assert native.consistency_launches() == launches + 4                 # the host path launches nothing
    fa, fb = consistency_files(a), consistency_files(b)
    assert len(fa) == 8 and fa == fb
    for i in range(4):
        for f in ("depth.npy", "normal.npy", "weak.npy"):
            pa, pb = (os.path.join(d, "DPE", f"{i:08d}", f) for d in (a, b))
            assert open(pa, "rb").read() == open(pb, "rb").read(), (i, f)
        count = np.load(os.path.join(a, "DPE", f"{i:08d}", "consistency.npy"))
        assert count.dtype == np.uint8 and count.shape == (48, 64)
    assert open(os.path.join(a, "DPE", "DPE.ply"), "rb").read() == open(os.path.join(b, "DPE", "DPE.ply"), "rb").read()
    assert any(0 < np.count_nonzero(np.load(os.path.join(a, "DPE", f"{i:08d}", "consistency.npy"))) < 64 * 48 for i in range(4))


# ------------------------------------------------------------------------------ 10. off
def test_consistency_off_launches_nothing(tmp_path, dense4):
    a = _copy(dense4, tmp_path, "off")
    launches, live = native.consistency_launches(), native.live_device_bytes()
    assert pipeline.run_dpe_pipeline(a, normal=True, weak=True, verbose=False, consistency=0) == 0
    assert native.consistency_launches() == launches and native.live_device_bytes() == live
    names = [f for _, _, fs_ in os.walk(os.path.join(a, "DPE")) for f in fs_]
    assert "depth.npy" in names and "consistency.npy" not in names and "depth_filtered.npy" not in names
