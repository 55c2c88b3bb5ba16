"""The fast taps' texel offset (csrc/tex_addr.h) on the GPU: passes whose patches reach the texel
arrays' borders through every tap path, bit-exact against the CPU oracle (tolerance 0 on planes,
weak, sel and costs, as test_gpu_parity.py).

  * REFINE_ITER + geometric consistency at 80x60 with 3 views whose source cameras' principal points
    are moved, so that a good share of the reference patches project across the source image's border
    (clamped taps, texel indices 0 and lim + 1) and the rest inside (clamp-free taps); at this size the
    strong pools' last rounds are split tails.  Once with 8-bit images (strong sweep TEX_P16,
    DepthToWeak / LocalRefine TEX_F16, weak sweep TEX_U8) and once with quarter-integer ones (weak
    sweep TEX_F16).
  * W = 8190, the first width whose TEX_F16 rows pass 65535 bytes: that layout's kernels run with the
    four-instruction offset (TEX_F16W), the 4-byte layouts with the packed one at a 32772-byte row.
    H = 14 leaves DepthToWeak two interior rows; 2 views and one iteration keep the oracle to seconds.
"""
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


def assert_same(g, o, what):
    for k in ("planes", "weak", "sel", "costs"):
        if not bits_equal(g[k], o[k]):
            a, b = g[k], o[k]
            neq = (a.view(np.uint32) != b.view(np.uint32)) if a.dtype == np.float32 else (a != b)
            if neq.ndim == 3:
                neq = neq.any(-1)
            ys, xs = np.nonzero(neq)
            pytest.fail(f"{what}: {k} differs at {len(ys)} pixels, first ({ys[0]}, {xs[0]})")


def _refine_iter(iters):
    p = _abi.default_params()
    p.max_iterations = iters
    p.state = _abi.REFINE_ITER; p.geom_consistency = True; p.rotate_time = 2; p.ransac_threshold = 0.00875
    p.max_scale_size = 2; p.weak_peak_radius = 2
    return p


def _quarter(W, H, N):
    """the scene at W x H with the host pipeline's 1/2 downscale of its 2W x 2H images (multiples of 1/4)"""
    from DPE_MVS import pipeline
    full = synthetic.make_scene(2 * W, 2 * H, N)
    sc = synthetic.make_scene(W, H, N)
    sc["images"] = [pipeline.resize_linear(im.astype(np.float32), W, H) for im in full["images"]]
    q = np.concatenate([im.ravel() for im in sc["images"]])
    assert np.all(q * 4 == np.round(q * 4)) and not np.all(q == np.round(q))
    return sc


def _projected_centres(sc, v):
    """reference pixels projected into source view v at their ground-truth depth, with the pass's camera"""
    W, H = sc["W"], sc["H"]
    v0, vs = sc["views"][0], sc["views"][v]
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.where(np.isfinite(v0["depth"]), v0["depth"], 5.0)
    X = (np.linalg.inv(v0["K"]) @ np.stack([xs.ravel(), ys.ravel(), np.ones(W * H)])) * d.ravel()
    Xw = v0["R"].T @ (X - v0["t"][:, None])
    Ks = np.array(list(sc["cams"][v].K), float).reshape(3, 3)
    p = Ks @ (vs["R"] @ Xw + vs["t"][:, None])
    return p[0] / p[2], p[1] / p[2]


@pytest.mark.parametrize("kind,cls", [("u8", 2), ("quarter", 1)])
def test_patches_across_the_image_border(ctx, kind, cls):
    W, H, N = 80, 60, 3
    sc = synthetic.make_scene(W, H, N) if kind == "u8" else _quarter(W, H, N)
    # principal points moved: view 1 a third of the width to the left, view 2 a third of the height down
    sc["cams"][1].K[2] -= W / 3.0
    sc["cams"][2].K[5] += H / 3.0
    for v, lim_x, lim_y in ((1, W, H), (2, W, H)):
        x, y = _projected_centres(sc, v)
        inside = (x >= 0) & (x < lim_x) & (y >= 0) & (y < lim_y)
        # patches (radius 5) that straddle the border: centre inside, a tap outside
        straddle = inside & ((x < 6) | (x > lim_x - 7) | (y < 6) | (y > lim_y - 7))
        clear = inside & ~straddle
        assert straddle.mean() > 0.10 and clear.mean() > 0.25, (v, straddle.mean(), clear.mean())
    p = _refine_iter(3)
    st = synthetic.gt_state(sc, seed=W + H)
    inp = synthetic.pass_input(sc, p, depths=synthetic.src_depths(sc), seed=W * 7 + N)
    assert_same(ctx.run(inp, st), oracle.run_pass(inp, st), f"{W}x{H}x{N} {kind}, shifted source cameras")
    assert ctx.last_stat(_abi.DPE_STAT_TEX_CLASS) == cls


@pytest.mark.parametrize("kind,cls", [("u8", 2), ("quarter", 1)])
def test_first_width_over_the_packed_limit(ctx, kind, cls):
    W, H, N = 8190, 14, 2
    assert (W + 2) * 8 > 65535 >= (W + 1) * 8 and (W + 3) * 4 <= 65535
    sc = synthetic.make_scene(W, H, N) if kind == "u8" else _quarter(W, H, N)
    p = _refine_iter(1)
    st = synthetic.gt_state(sc, seed=W + H)
    inp = synthetic.pass_input(sc, p, depths=synthetic.src_depths(sc), seed=W * 7 + N)
    assert_same(ctx.run(inp, st), oracle.run_pass(inp, st), f"{W}x{H}x{N} {kind}")
    assert ctx.last_stat(_abi.DPE_STAT_TEX_CLASS) == cls
