"""Inputs of the rare-tap-path tests (test_scaled_camera_inputs.py on the oracle, test_gpu_scaled_cameras.py
on the device): synthetic scenes whose source cameras have all nine entries of K multiplied by a constant.

The homography H = M_v - b_v g^T is homogeneous in the source K, so qx, qy and qz of every tap scale
together and the projected point does not move; under a power-of-two (or negated) scale no rounding changes
either, as long as nothing under- or overflows.  What changes is the branch a kernel takes: the whole-patch
reciprocal range test (csrc/pass_common.h rcp_range_ok) wants qz of one sign inside 2^-100 .. 2^100, and
the tap reciprocal is the IEEE quotient outside biased exponents 1..252 (device_math.h rcp_model).
DESIGN.md §4, row "rare tap paths".
"""
import functools

import numpy as np

import oracle
from DPE_MVS import _abi, synthetic
from test_gpu_parity import _params

P = lambda e: 2.0 ** e  # noqa: E731

# name -> scales of the source views, cycled: view v (1..N-1) takes scales[(v - 1) % len(scales)]
SCALE_SETS = {
    # A1: every patch box fails the range test (16x beyond its 2^+-100 bounds), nothing rounds differently
    "A1_small": [P(-104)], "A1_large": [P(104)], "A1_small_negative": [-P(-104)],
    # A2: the range test passes with a negative denominator everywhere
    "A2_negative": [-1.0],
    # A3: fast and slow patches in the same pools, tails and ballots
    "A3_large_plain": [P(104), 1.0], "A3_negative_small_plain": [-1.0, P(-104), 1.0],
    # B: denormal third row of K, qz at or below the normal range: the IEEE reciprocal, finite taps
    "B_denormal_plain": [P(-127), 1.0], "B_min_normal": [P(-126)],
    # C: 1/qz overflows (2^-129: view dead); 2^116: slow, and homography rows near 2^123, so a numerator
    # overflows where a hypothesis projects ~2^5 image widths away; 2^126: the focal lengths overflow to inf
    # (every tap of the view NaN) and qz >= 2^126 (the IEEE reciprocal on the large side)
    "C_dead_plain_overflow": [P(-129), 1.0, P(116)], "C_dead_plain_inf": [P(-129), 1.0, P(126)],
    "C_all_dead": [P(-129)],
}
EXACT_SETS = [k for k in SCALE_SETS if k[0] == "A"]   # outputs bit-identical to the unscaled pass (photometric)

# name -> (W, H, views, kind of test_gpu_parity._params, iterations, parameter overrides)
CONFIGS = {
    "iter_80x60": (80, 60, 4, "refine_iter", 3, {}),       # split pool tails, 16-lane edge scheme, WEAK pixels
    "first_80x60": (80, 60, 4, "first", 3, {}),            # 8-lane ACMH kernel, random init over all views
    "init_80x60": (80, 60, 4, "refine_init", 3, {}),
    "acmh_57x43": (57, 43, 3, "acmh_geom", 2, {}),         # ragged waves
    "weak_generic_72x56": (72, 56, 3, "weak_generic", 3, {}),   # untabulated NCC-New
    "radius4_64x48": (64, 48, 3, "first", 1, dict(strong_radius=4, strong_increment=1)),   # patch_ncc_generic
    "no_limit_80x60": (80, 60, 4, "no_limit", 3, {}),
    "fused_40x13": (40, 13, 3, "refine_iter", 3, {}),      # fused DepthToWeak + LocalRefine beside the border kernel
    "border_12x40": (12, 40, 3, "refine_iter", 3, {}),     # LocalRefine's border kernel over every pixel
    "lowres_72x54": (72, 54, 5, "refine_iter_lowres", 3, {}),   # labels, low-res
}
MAIN_CONFIGS = ["iter_80x60", "first_80x60"]               # every scale set, every texel class
OTHER_CONFIGS = [c for c in CONFIGS if c not in MAIN_CONFIGS]
OTHER_SETS = ["A1_small", "A3_negative_small_plain", "C_dead_plain_overflow", "C_dead_plain_inf"]   # on the other configs, 8-bit images
PHOTOMETRIC = [c for c, v in CONFIGS.items() if v[3] in ("first", "refine_init", "no_limit")]
TEXEL_CLASS = {"u8": 2, "quarter": 1, "f32": 0}            # DPE_STAT_TEX_CLASS of each


def views_of(config, set_name):
    """C_all_dead runs with 3 views (2 sources, both dead) whatever the config's count."""
    return 3 if set_name == "C_all_dead" else CONFIGS[config][2]


def scale_K(scene, scales):
    """The scene with the nine K entries of source view v (v = 1..N-1) multiplied by
    np.float32(scales[(v - 1) % len(scales)]).  R, t, c, the size and the depth range stay; view 0 is never
    scaled (the kernels take cams[0].K[8] = 1 for granted: kinv0, depth_from_plane)."""
    cams = [_abi.DpeCamera.from_buffer_copy(c) for c in scene["cams"]]
    for v in range(1, len(cams)):
        s = np.float32(scales[(v - 1) % len(scales)])
        with np.errstate(over="ignore"):          # 2^126: the focal lengths become inf, on purpose
            for i in range(9):
                cams[v].K[i] = float(np.float32(cams[v].K[i]) * s)
    return dict(scene, cams=cams)


@functools.lru_cache(maxsize=None)
def texel_scene(W, H, N, texel):
    """The W x H, N-view scene with its grey levels in a texel class, built as test_gpu_parity._texel_scene
    builds them: "u8" integers, "quarter" the INTER_LINEAR half-size of the 2W x 2H scene (multiples of 1/4),
    "f32" neither.  Callers do not modify them."""
    sc = synthetic.make_scene(W, H, N)
    if texel == "quarter":
        from DPE_MVS import pipeline
        full = synthetic.make_scene(2 * W, 2 * H, N)
        images = [pipeline.resize_linear(im.astype(np.float32), W, H) for im in full["images"]]
        q = np.concatenate([im.ravel() for im in images])
        assert np.all(q * 4 == np.round(q * 4)) and not np.all(q == np.round(q))
        sc = dict(sc, images=images)
    elif texel == "f32":
        sc = dict(sc, images=[(im * np.float32(0.73) + np.float32(0.31)).astype(np.float32) for im in sc["images"]])
    else:
        assert texel == "u8"
    return sc


def case(config, set_name=None, texel="u8"):
    """(pass input, state, label) of a config with the scale set applied (None: the unscaled cameras)."""
    W, H, _, kind, iters, over = CONFIGS[config]
    N = views_of(config, set_name)
    sc = texel_scene(W, H, N, texel)
    if set_name is not None:
        sc = scale_K(sc, SCALE_SETS[set_name])
    p = _params(kind, iters)
    for k, v in over.items():
        setattr(p, k, v)
    st = synthetic.first_init_state(sc) if kind == "first" else synthetic.gt_state(sc, seed=W + H)
    inp = synthetic.pass_input(sc, p, depths=synthetic.src_depths(sc) if p.geom_consistency else None, seed=W * 7 + N)
    return inp, st, f"{config} x{N} {texel} K*{set_name}"


def pairs():
    """The (config, scale set, texel class) cases of the two test modules."""
    out = [(c, s, t) for c in MAIN_CONFIGS for s in SCALE_SETS for t in TEXEL_CLASS]
    out += [(c, s, "u8") for c in OTHER_CONFIGS for s in OTHER_SETS]
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(config, set_name=None, texel="u8"):
    """(outputs, tap-path class counts) of the oracle's pass over case(...).  Shared; callers do not modify."""
    inp, st, _ = case(config, set_name, texel)
    out = oracle.run_pass(inp, st)
    return out, oracle.last_tap_stats()
