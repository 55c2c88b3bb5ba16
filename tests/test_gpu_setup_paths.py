"""GPU parity of the set-up work around the 36-tap loops: the pass-constant tables
(PassConst::base_len / ::spat36), the strong sweep's slot lists, selected-view lists and refinement
hypotheses built on several lanes of a pixel instead of one, and the last rounds of its two job
pools split by patch rows (csrc/pool_tail.h).  Every output (planes, weak, sel, costs) must be the
CPU oracle's bit for bit: the oracle keeps the per-pixel, one-thread form of all of these.

The view counts 2..10 give the job pools last rounds of many sizes and the view ballots many fill
levels (10 images = 9 source views: more views than the 8 lanes an ACMH pixel has), 57x43 leaves
ragged waves and rows, and both candidate schemes run (edge: 16 lanes per pixel, ACMH: 8).  The f32
cases (images that are neither 8-bit nor quarter-integer) run the f32-texel instantiations, where the
strong sweep builds its slot list and refinement hypotheses on one lane and its tails stay narrow."""
import numpy as np
import pytest

import oracle
from DPE_MVS import _abi, synthetic
from golden_io import bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from DPE_MVS import native
    c = native.PatchMatchContext(0)
    yield c
    c.close()


def _params(kind):
    p = _abi.default_params()
    p.max_iterations = 2
    p.state = _abi.REFINE_ITER
    p.geom_consistency = True
    p.rotate_time = 2
    p.ransac_threshold = 0.00875
    if kind == "refine_iter":            # the edge scheme
        p.max_scale_size = 2; p.weak_peak_radius = 2
    else:                                # "acmh_geom": ACMH candidates (no APD / edges)
        p.use_APD = False; p.use_edge = False
    return p


def _assert_same(g, o, what):
    for k in ("planes", "weak", "sel", "costs"):
        if not bits_equal(g[k], o[k]):
            a, b = g[k], o[k]
            neq = (a.view(np.uint32) != b.view(np.uint32)) if a.dtype == np.float32 else (a != b)
            if neq.ndim == 3:
                neq = neq.any(-1)
            ys, xs = np.nonzero(neq)
            pytest.fail(f"{what}: {k} differs at {len(ys)} pixels, first ({ys[0]}, {xs[0]})")


def _run(ctx, W, H, N, p, what, tex="u8"):
    sc = synthetic.make_scene(W, H, N)
    if tex == "f32":                     # grey levels off the 1/4 grid, as test_gpu_non_integer_images makes them
        sc["images"] = [(im * np.float32(0.73) + np.float32(0.31)).astype(np.float32) for im in sc["images"]]
    st = synthetic.gt_state(sc, seed=W + H)
    inp = synthetic.pass_input(sc, p, depths=synthetic.src_depths(sc), seed=W * 7 + N)
    _assert_same(ctx.run(inp, st), oracle.run_pass(inp, st), what)
    if tex == "f32":
        assert ctx.last_stat(_abi.DPE_STAT_TEX_CLASS) == 0, f"{what}: not the f32-texel kernels"


_CASES = [pytest.param(kind, W, H, N, "u8", id=f"{kind}-{W}-{H}-{N}")
          for kind in ("refine_iter", "acmh_geom") for W, H in ((64, 48), (57, 43)) for N in (2, 3, 4, 6, 10)]
_CASES += [pytest.param(kind, 57, 43, N, "f32", id=f"{kind}-57-43-{N}-f32")
           for kind in ("refine_iter", "acmh_geom") for N in (3, 10)]


@pytest.mark.parametrize("kind,W,H,N,tex", _CASES)
def test_setup_paths_match_oracle(ctx, kind, W, H, N, tex):
    _run(ctx, W, H, N, _params(kind), f"{W}x{H}x{N} {kind} {tex}", tex)


def test_spatial_table_follows_sigma(ctx):
    # non-default sigmas at the default 5/2 patch: spat36 is built from the pass's sigma_spatial
    p = _params("refine_iter")
    p.sigma_spatial = 4.0
    p.sigma_color = 6.0
    _run(ctx, 64, 48, 4, p, "64x48x4 refine_iter sigma 4 / 6")
