"""The conditions that keep tests/test_gpu_scaled_cameras.py honest, measured on the oracle alone.

That module runs passes whose source cameras have K multiplied by a constant (scaled_cameras.py) and
compares the device with the oracle bit for bit.  It only means something if (i) the scaled inputs really send
the patches and taps down the kernels' rare branches, (ii) the scaled views are still used by the pass (a
view that is never selected tests nothing), and (iii) where the construction is exact the oracle's own outputs
do not move.  Each is asserted here, per (config, scale set), from the oracle's outputs and from its
tap-path class counts (oracle.last_tap_stats: the kernels' whole-patch range test transcribed in float32 over
the restatement's own homographies, and the class of every tap).

What the sets are and are not, by construction (measured; the figures are in DESIGN.md §4):
 * A 2^-129 view never reaches a tap: every NCC of it ends at the centre test (1 / qz = inf, the centre is
   "outside"; C_all_dead: 0 patches).
 * A 2^116 view is a slow view like A1's and as much in use (selected on ~0.75 of the pixels), with qz near
   2^116 (inside the reciprocal table) and homography rows near 2^123: a numerator overflows only where a
   hypothesis projects some 2^5 image widths away (a few dozen NaN taps per pass, none on some configs).
   The share of 0.33-0.36 once measured for it was the oracle's: it scaled the numerators by 256 before the
   coordinate FMA, which overflowed in-image taps that the kernels (and the reference's q / qz) compute
   finite; the scaled-camera parity test found that, and the oracle now takes the unscaled numerator.
 * The 2^126 view is what that figure described: focal lengths inf, every tap of the view NaN (texel 0 by the
   clamp's NaN rule), qz >= 2^126 (IEEE reciprocal), still selected on 0.1 .. 0.6 of the pixels.  All three
   tap counts are > 0 there.
 * A config with 3 views has no third scale (the scales cycle over 2 sources): its C cases are "one dead
   view" only.
 * A2's patches do not all pass the range test: the few whose box fails it with unscaled cameras (a
   denominator that crosses zero or spans > 2^20 over the box: 90 of 1.57e6 at 80x60) fail it negated
   too.  None takes the positive side.
"""
import numpy as np
import pytest

import scaled_cameras as sc
from golden_io import bits_equal

U8_PAIRS = [(c, s) for c, s, t in sc.pairs() if t == "u8"]
OUT = ("planes", "weak", "sel", "costs")


def _share(sel, v):
    return float(((sel >> np.uint32(v - 1)) & 1).mean())


def _scaled_views(config, set_name):
    """(view, scale) of the source views whose scale is not 1."""
    scales = sc.SCALE_SETS[set_name]
    vs = [(v, scales[(v - 1) % len(scales)]) for v in range(1, sc.views_of(config, set_name))]
    return [(v, s) for v, s in vs if s != 1.0]


def test_scale_K_touches_only_source_K():
    scene = sc.texel_scene(80, 60, 4, "u8")
    scaled = sc.scale_K(scene, [2.0 ** 104, -1.0])
    for v, (a, b) in enumerate(zip(scene["cams"], scaled["cams"])):
        s = (1.0, 2.0 ** 104, -1.0, 2.0 ** 104)[v]
        assert [x * s for x in a.K] == list(b.K), v
        for f in ("R", "t", "c"):
            assert list(getattr(a, f)) == list(getattr(b, f)), (v, f)
        assert (a.width, a.height, a.depth_min, a.depth_max) == (b.width, b.height, b.depth_min, b.depth_max)
    assert scaled["cams"][0] is not scene["cams"][0] and scaled["images"] is scene["images"]
    # 2^-127 leaves the third row of K denormal, not zero
    tiny = sc.scale_K(scene, [2.0 ** -127])
    assert tiny["cams"][1].K[8] == 2.0 ** -127 and tiny["cams"][1].K[0] == scene["cams"][1].K[0] * 2.0 ** -127


EXACT_PAIRS = [(c, s, t) for c, s, t in sc.pairs() if c in sc.PHOTOMETRIC and s in sc.EXACT_SETS and t != "quarter"]


@pytest.mark.parametrize("config,set_name,texel", EXACT_PAIRS)
def test_exact_sets_leave_the_photometric_oracle_pass_unchanged(config, set_name, texel):
    """A1 / A2 / A3 on the photometric passes: the oracle's outputs with scaled cameras are the unscaled
    pass's bits (the geometric term assumes K[8] = 1 in world_point / project_cam: not asserted there)."""
    got, _ = sc.oracle_case(config, set_name, texel)
    want, _ = sc.oracle_case(config, None, texel)
    for k in OUT:
        assert bits_equal(got[k], want[k]), k


@pytest.mark.parametrize("config,set_name", U8_PAIRS)
def test_scaled_views_are_used(config, set_name):
    """A and B: every scaled view selected on at least half of the pixels, costs < 2 on at least 0.75 of them.
    C: the 2^-129 views selected nowhere, the 2^126 view on 0.1 .. 0.6 of the pixels, the 2^116 view like
    A's (see the module docstring); with every source dead
    nothing is selected and no view gave a cost: every cost NaN on the first pass, NaN or the "no cost" 2.0 on
    a refine pass (its costs of the prior's WEAK and UNKNOWN pixels: 1609 of 4800 at 80x60)."""
    out, _ = sc.oracle_case(config, set_name)
    sel, costs = out["sel"], out["costs"]
    shares = {v: _share(sel, v) for v, _ in _scaled_views(config, set_name)}
    print(f"{config} K*{set_name}: sel share of the scaled views {shares}, costs < 2 on {float((costs < 2).mean()):.3f}")
    if set_name == "C_all_dead":
        assert not sel.any() and (np.isnan(costs) | (costs == 2.0)).all() and np.isnan(costs).mean() > 0.5
        if sc.CONFIGS[config][3] == "first":
            assert np.isnan(costs).all()
        return
    for v, s in _scaled_views(config, set_name):
        if s == 2.0 ** -129:
            assert shares[v] == 0.0, (v, shares)
        elif s == 2.0 ** 126:
            assert 0.1 <= shares[v] <= 0.6, (v, shares)
        else:
            assert shares[v] >= 0.5, (v, shares)
    if set_name[0] in "AB":
        assert float((costs < 2).mean()) >= 0.75


@pytest.mark.parametrize("config,set_name", U8_PAIRS)
def test_tap_path_class_counts(config, set_name):
    """Which branches the scaled inputs reach, from the oracle's class counts (see the module docstring
    for A2 and C)."""
    _, n = sc.oracle_case(config, set_name)
    print(f"{config} K*{set_name}: {n}")
    patches, slow, negative = n["patches"], n["patches_slow"], n["patches_negative"]
    assert slow + negative <= patches
    if set_name == "C_all_dead":
        assert patches == 0            # every NCC ends at the centre test
        return
    assert patches > 0
    if set_name.startswith("A1"):
        assert slow == patches         # every NCC evaluation that reaches the taps is slow
    elif set_name.startswith("A2"):
        assert slow + negative == patches and negative > slow     # none on the positive side
        if config in sc.PHOTOMETRIC:   # the same pass as unscaled: the same few boxes fail the test
            assert slow == sc.oracle_case(config, None)[1]["patches_slow"]
    elif set_name.startswith("A3"):
        assert 0 < slow < patches      # the scaled views' boxes fail, the unscaled view's pass
        if "negative" in set_name:
            assert negative > 0
            if sc.views_of(config, set_name) >= 4:      # the third source is the unscaled one
                assert slow + negative < patches
    if set_name[0] == "A":
        assert n["taps_ieee_rcp"] == 0 and n["taps_nan"] == 0
    elif set_name[0] == "B":
        assert n["taps_ieee_rcp"] > 0 and n["taps_nan"] == 0
    else:
        assert n["taps_clamped"] > 0
        if any(s == 2.0 ** 126 for _, s in _scaled_views(config, set_name)):
            assert n["taps_ieee_rcp"] > 0 and n["taps_nan"] > 0
        else:
            assert n["taps_ieee_rcp"] == 0


@pytest.mark.parametrize("config", list(sc.CONFIGS))
def test_unscaled_scenes_hardly_reach_the_slow_branches(config):
    """The gap: with the cameras of synthetic.make_scene the share of patches on the slow branch (printed, not
    asserted), none on the negative side, no tap outside the reciprocal table, none NaN."""
    _, n = sc.oracle_case(config, None)
    print(f"{config} unscaled: {n['patches_slow']} of {n['patches']} patches slow "
          f"({n['patches_slow'] / max(1, n['patches']):.2e}); {n}")
    assert n["patches"] > 0 and n["patches_negative"] == 0 and n["taps_ieee_rcp"] == 0 and n["taps_nan"] == 0


def test_counts_are_the_same_on_one_thread_and_on_many():
    import oracle
    inp, st, _ = sc.case("fused_40x13", "C_dead_plain_overflow")
    a = oracle.run_pass(inp, st, threads=1)
    one = oracle.last_tap_stats()
    b = oracle.run_pass(inp, st, threads=5)
    many = oracle.last_tap_stats()
    assert one == many and one["patches"] > 0
    for k in OUT:
        assert bits_equal(a[k], b[k]), k
