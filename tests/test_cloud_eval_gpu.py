"""Cloud evaluation on the device (csrc/pass_cloud.h, dpe_cloud_nn / dpe_cloud_nn_pair of include/dpe_mvs.h):
the kernels must give the host path's distances bit for bit on every cloud of tests/test_cloud_eval.py (where
the host path is pinned against a brute-force loop) and on 100 000 x 100 000 clustered points, the same bits
on every run, the host path's dict and table through evaluate_clouds and bin/dpe_eval, and a pipeline run
must launch none of them.  One end-to-end case scores a fused cloud against the scene's ground truth."""
import os
import subprocess

import numpy as np
import pytest

from DPE_MVS import native, pipeline, synthetic
from test_cloud_eval import CLOUDS, F, PKG, cloud_case, eval_files, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.PatchMatchContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------ 1. device against host
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_device_matches_host_and_brute(ctx, name):
    Q, T, R, want = cloud_case(name)
    got = ctx.cloud_nn(Q, T, R)
    assert same_bits(got, pipeline.cloud_nn(Q, T, R)) and same_bits(got, want)
    back = ctx.cloud_nn(T, Q, R)                                          # the other direction: the queries as the grid
    assert same_bits(back, pipeline.cloud_nn(T, Q, R))
    ab, ba = ctx.cloud_nn_pair(Q, T, R)                                   # the pair = two single calls
    assert same_bits(ab, got) and same_bits(ba, back)


@pytest.mark.parametrize("n,m", [(0, 5), (5, 0), (1, 1), (0, 0)])
def test_degenerate_sizes(ctx, n, m):
    rng = np.random.default_rng(1)
    Q, T = rng.random((n, 3)).astype(F), rng.random((m, 3)).astype(F)
    before = native.cloud_launches()
    got = ctx.cloud_nn(Q, T, 0.5)
    assert same_bits(got, pipeline.cloud_nn(Q, T, 0.5))
    ab, ba = ctx.cloud_nn_pair(Q, T, 0.5)
    assert same_bits(ab, got) and same_bits(ba, pipeline.cloud_nn(T, Q, 0.5))
    if n == 0 and m == 0:
        assert native.cloud_launches() == before                         # nothing to do: nothing launched
    only_bad = np.full((3, 3), np.nan, F)
    assert (ctx.cloud_nn(T, only_bad, 0.5) == F(0.25)).all()              # no finite target: all R2


def clustered(seed, n):
    """n points in 40 clusters of very different density over a 10 x 10 x 2 slab (the same clusters for every
    seed), 50 of them far outliers."""
    rng = np.random.default_rng(77)
    centres = rng.random((40, 3)) * [10, 10, 2]
    sigma = 10.0 ** rng.uniform(-2.5, -0.5, 40)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 40, n)
    p = centres[k] + rng.normal(0, 1, (n, 3)) * sigma[k][:, None]
    p[:50] = rng.uniform(-500, 500, (50, 3))
    return p.astype(F)


def test_device_matches_host_on_100k_clustered_points(ctx):
    A, B, R = clustered(1, 100_000), clustered(2, 100_000), 0.02
    want_ab, want_ba = pipeline.cloud_nn(A, B, R), pipeline.cloud_nn(B, A, R)
    ab, ba = ctx.cloud_nn_pair(A, B, R)
    assert same_bits(ab, want_ab) and same_bits(ba, want_ba)
    share = float((ab < F(R) * F(R)).mean())
    print("100k clustered: untruncated share", share)
    assert 0.02 < share < 0.98
    again_ab, again_ba = ctx.cloud_nn_pair(A, B, R)                       # two device runs: equal bits
    assert same_bits(again_ab, ab) and same_bits(again_ba, ba)
    assert same_bits(ctx.cloud_nn(A, B, R), ab)


# ------------------------------------------------------------------------------ 2. errors, memory
def test_argument_errors_and_memory():
    live = native.live_device_bytes()
    c = native.PatchMatchContext(0)
    try:
        Q, T, R, _ = cloud_case("random")
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(native.DpeError, match=r"\(-1\).*bad argument"):  # DPE_ERR_ARG
                c.cloud_nn(Q, T, bad)
            with pytest.raises(native.DpeError, match=r"\(-1\).*bad argument"):
                c.cloud_nn_pair(Q, T, bad)
        far = np.array([[-1e30, 0, 0], [1e30, 0, 0]], F)
        with pytest.raises(native.DpeError, match=r"\(-1\).*radius too small for the cloud's extent"):
            c.cloud_nn(Q, far, 1e-3)
        with pytest.raises(native.DpeError, match=r"\(-1\).*radius too small for the cloud's extent"):
            c.cloud_nn_pair(far, Q, 1e-3)
        assert same_bits(c.cloud_nn(far, T, R), pipeline.cloud_nn(far, T, R))        # far QUERIES are fine
        out = np.empty(len(Q), F)
        lib = native._LIB
        assert lib.dpe_cloud_nn(c._ctx, Q.ctypes.data, 2 ** 31, T.ctypes.data, len(T), 0.25, out.ctypes.data) == -1
        assert lib.dpe_cloud_nn(c._ctx, None, len(Q), T.ctypes.data, len(T), 0.25, out.ctypes.data) == -1
        assert lib.dpe_cloud_nn(c._ctx, Q.ctypes.data, len(Q), T.ctypes.data, len(T), 0.25, None) == -1
        assert lib.dpe_cloud_nn(None, Q.ctypes.data, len(Q), T.ctypes.data, len(T), 0.25, out.ctypes.data) == -1
        assert same_bits(c.cloud_nn(Q, T, R), cloud_case("random")[3])               # still usable after the refusals
        assert native.live_device_bytes() > live
    finally:
        c.close()
    assert native.live_device_bytes() == live                             # the context gave everything back


# ------------------------------------------------------------------------------ 3. the evaluation through the device
def test_evaluate_on_the_device_gives_the_host_dict_and_table(tmp_path):
    recon, gt, taus, want = eval_files(tmp_path)
    Q, T, _, _ = cloud_case("random")
    live = native.live_device_bytes()
    assert pipeline.evaluate_clouds(Q, T, taus, radius=0.25, gpu_index=0) == want
    assert native.live_device_bytes() == live                             # its own context, closed again
    Qn, Tn, R, _ = cloud_case("nonfinite")
    assert pipeline.evaluate_clouds(Qn, Tn, [0.1, R], gpu_index=0) == pipeline.evaluate_clouds(Qn, Tn, [0.1, R])
    with pytest.raises(pipeline.PipelineError, match="radius too small for the cloud's extent"):
        pipeline.evaluate_clouds(Q, np.array([[-1e30, 0, 0], [1e30, 0, 0]], F), [1e-3], gpu_index=0)
    r = subprocess.run([os.path.join(PKG, "bin", "dpe_eval"), recon, gt] + [repr(t) for t in taus] +
                       ["--radius", "0.25", "--gpu", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == pipeline.format_cloud_eval(want)


# ------------------------------------------------------------------------------ 4. end to end
def test_fused_cloud_against_the_scenes_ground_truth(tmp_path):
    """A 64 x 48, 4-view synthetic dense folder through the pipeline with fusion, then DPE/DPE.ply against
    synthetic.gt_point_cloud at tau = 1, 2, 4, 8 pixel footprints (5 / fx).  No F-score is fixed: it must rise
    with tau, beat the same cloud shifted by 10 tau_max (which scores 0), and the pipeline itself must launch no
    kernel of the evaluation.  Measured on an MI355X: F = 0.1803, 0.3579, 0.5923, 0.7790
    (177 fused points: precision 0.92 to 1.00, recall 0.10 to 0.64)."""
    d = str(tmp_path / "dense")
    sc = synthetic.write_dense_folder(d, 64, 48, 4)
    before = native.cloud_launches()
    assert pipeline.run_dpe_pipeline(d, verbose=False, fusion=True) == 0
    assert native.cloud_launches() == before                              # the pipeline launched none
    recon = pipeline.read_point_cloud(os.path.join(d, "DPE", "DPE.ply"))
    gt = synthetic.gt_point_cloud(sc)
    assert len(recon) > 100 and len(gt) == 4 * 64 * 48
    foot = 5.0 / (1.2 * 64)
    taus = [foot, 2 * foot, 4 * foot, 8 * foot]
    e = pipeline.evaluate_clouds(recon, gt, taus, gpu_index=0)
    assert native.cloud_launches() > before
    print("end to end: F =", e["fscore"], "precision", e["precision"], "recall", e["recall"], "points", len(recon))
    assert e == pipeline.evaluate_clouds(recon, gt, taus)
    f = e["fscore"]
    assert all(f[k] <= f[k + 1] for k in range(3)) and f[3] > 0.0
    shifted = pipeline.evaluate_clouds(recon + F(10 * taus[3]), gt, taus, gpu_index=0)
    assert shifted["fscore"] == [0.0] * 4 and f[3] > shifted["fscore"][3]
