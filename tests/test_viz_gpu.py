"""The viz medium results on the device (csrc/pass_viz.h, dpe_state_render* of include/dpe_mvs.h): the
render kernel and the JPEG front-half kernel must equal the host functions bit for bit (they are
checked against numpy and libjpeg in tests/test_viz.py), the resident pipeline must write the same
files as the host path, and a run with viz = false must launch none of the new kernels."""
import os

import numpy as np
import pytest

from DPE_MVS import _abi, native, pipeline, synthetic
from test_pipeline import oracle_runner, _copy
from test_viz import (COLOUR_SHAPES, check_viz_folder, depth_kat_inputs, jpgs_under, noisy_gradient_bgr,
                      normal_kat_inputs, remove_maps_of_image0)

pytestmark = pytest.mark.gpu
KINDS = (pipeline.VIZ_DEPTH, pipeline.VIZ_NORMAL, pipeline.VIZ_WEAK)


@pytest.fixture(scope="module")
def ctx():
    c = native.PatchMatchContext(0)
    yield c
    c.close()


def host_pictures(state, dmin, dmax):
    return [pipeline.viz_render(k, depth=state["depth"], normal=state["normal"], weak=state["weak"], dmin=dmin, dmax=dmax)
            for k in KINDS]


# ------------------------------------------------------------------------------ 5. render, device vs host
@pytest.mark.parametrize("W,H", [(64, 48), (50, 33)])
def test_state_render_matches_host(ctx, W, H):
    """One small pass + dpe_state_save: the real post-epilogue state (with depths sent to 0 / UNKNOWN)."""
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
    ctx.state_save(11)
    state = ctx.state_fetch(11)
    assert state["depth"].shape == (H, W)
    assert (state["weak"] == _abi.UNKNOWN).any()
    want = host_pictures(state, p.depth_min, p.depth_max)
    for k in KINDS:
        got = ctx.state_render(11, k, p.depth_min, p.depth_max)
        assert got.shape == (H, W, 3) and np.array_equal(got, want[k]), k
        # render + front half from the state == the host's front half of the host's picture
        assert np.array_equal(ctx.state_render_jpeg_blocks(11, k, p.depth_min, p.depth_max), pipeline.jpeg_blocks(want[k])), k
    assert len(np.unique(want[0].reshape(-1, 3), axis=0)) > 8      # the depth picture is not trivial
    # errors of the state entries
    with pytest.raises(native.DpeError, match=r"\(-4\).*no state"):   # DPE_ERR_STATE: unknown id
        ctx.state_render_jpeg_blocks(12345, pipeline.VIZ_DEPTH, 0, 1)
    with pytest.raises(native.DpeError, match=r"\(-1\).*bad kind"):   # DPE_ERR_ARG
        ctx.state_render_jpeg_blocks(11, 7, 0, 1)


def test_render_adversarial_values_match_host(ctx):
    """The KAT inputs of tests/test_viz.py through the same kernel (dpe_viz_render_arrays): range ends,
    NaN, the ramp's segment ends, the zero / NaN / non-unit normals, the rounding tie, every weak value."""
    d, dmin, dmax = depth_kat_inputs()
    n = normal_kat_inputs()
    m = 2 * len(d) + 3                                             # ragged: not a multiple of the 4-pixel stride
    depth = np.resize(d, (3, m)).astype(np.float32)
    normal = np.resize(n, (3 * m, 3)).reshape(3, m, 3).astype(np.float32)
    weak = (np.arange(3 * m) % 5).astype(np.uint8).reshape(3, m)
    weak[weak == 4] = 200
    assert np.array_equal(ctx.viz_render_arrays(pipeline.VIZ_DEPTH, depth=depth, dmin=dmin, dmax=dmax),
                          pipeline.viz_render(pipeline.VIZ_DEPTH, depth=depth, dmin=dmin, dmax=dmax))
    assert np.array_equal(ctx.viz_render_arrays(pipeline.VIZ_NORMAL, normal=normal), pipeline.viz_render(pipeline.VIZ_NORMAL, normal=normal))
    assert np.array_equal(ctx.viz_render_arrays(pipeline.VIZ_WEAK, weak=weak), pipeline.viz_render(pipeline.VIZ_WEAK, weak=weak))
    # dmin == dmax: 0 / 0 in the ramp, black on both
    flat = np.full((2, 5), 2.5, np.float32)
    assert not ctx.viz_render_arrays(pipeline.VIZ_DEPTH, depth=flat, dmin=2.5, dmax=2.5).any()
    assert not pipeline.viz_render(pipeline.VIZ_DEPTH, depth=flat, dmin=2.5, dmax=2.5).any()


# ------------------------------------------------------------------------------ 6. JPEG front half, device vs host
@pytest.mark.parametrize("shape", COLOUR_SHAPES + [(16, 16), (40, 100)])
def test_jpeg_front_half_matches_host(ctx, shape):
    """Width < 16, height < 16, sizes off the 8 and 16 grids (dummy blocks, replicated edges, the chroma
    rows below an even height's last one), several workgroups per row."""
    img = noisy_gradient_bgr(*shape)
    want = pipeline.jpeg_blocks(img)
    got = ctx.jpeg_blocks(img)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.abs(want).max() > 100                                # not a flat picture


# ------------------------------------------------------------------------------ 7. / 8. pipeline
@pytest.fixture(scope="module")
def dense4(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("vizgpu"))
    synthetic.write_dense_folder(d, 64, 48, 4)
    remove_maps_of_image0(d)
    return d


def test_resident_pipeline_writes_the_host_paths_files(tmp_path, dense4):
    a = _copy(dense4, tmp_path, "hip")
    b = _copy(dense4, tmp_path, "cpu")
    before = native.viz_launches()
    assert pipeline.run_dpe_pipeline(a, normal=True, weak=True, verbose=False, viz=True) == 0
    assert native.viz_launches() == before + 4 * 8 * 3 * 2         # render + front half per picture
    assert pipeline.run_dpe_pipeline(b, runner=oracle_runner(), normal=True, weak=True, verbose=False, viz=True) == 0
    names = check_viz_folder(b)
    assert jpgs_under(a) == jpgs_under(b) == sorted(names)
    for f in names:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    for i in range(4):
        for f in ("depth.npy", "normal.npy", "weak.npy"):
            assert open(os.path.join(a, "DPE", f"{i:08d}", f), "rb").read() == open(os.path.join(b, "DPE", f"{i:08d}", f), "rb").read()


def test_viz_off_launches_no_viz_kernel(tmp_path, dense4):
    a = _copy(dense4, tmp_path, "off")
    before = native.viz_launches()
    assert pipeline.run_dpe_pipeline(a, normal=True, weak=True, verbose=False, viz=False) == 0
    assert native.viz_launches() == before
    assert jpgs_under(a) == []
