"""GPU parity on the rare tap paths: source cameras with K multiplied by a constant (scaled_cameras.py).

Every pass kernel takes a bilinear tap in one of two ways: the fast path when the whole-patch test
(pass_common.h rcp_range_ok) proves the projective denominator qz of one sign inside 2^-100 .. 2^100, else the
slow path with a per-tap range test (rcp_tap<false> / rcp_model, tex_t's fmin(fmax) clamp with NaN -> low end,
sample_quad / sample_quad8, the rolled generic_taps loop).  On the scenes of synthetic.make_scene about
6 in 1e5 patches are slow and none has qz < 0, so the slow instantiations of each kernel and texel layout,
and the negative side of the fast path (sg = -1 in taps_unclamped, d_rcp_fast of negative denominators), ran
by accident if at all.  Scaling all of K of a source view by s scales qx, qy, qz together and moves no projected
point; it chooses the branch for every patch of that view:

  A1  s = 2^-104, 2^104, -2^-104     every patch slow, bit-exact construction
  A2  s = -1                         every patch on the fast path with qz < 0
  A3  mixes of those and 1           fast and slow jobs in the same pools, tails and ballots
  B   s = 2^-127, 2^-126             denormal / barely normal qz: the IEEE reciprocal, finite taps
  C   s = 2^-129, 2^116, 2^126       1 / qz = inf (dead views); rows near 2^123; focal lengths inf and
                                     qz >= 2^126: every tap of the view NaN

tests/test_scaled_camera_inputs.py asserts on the oracle alone that these inputs reach those branches and
that the scaled views stay in use.  Here every case must give the oracle's bits (tolerance 0 on planes, weak,
sel and costs), and for A on the photometric passes also the bits of the device's own pass with unscaled
cameras ("slow branch == fast branch", with no oracle involved).

Test ids start with setA / setB / setC so that the three can run one after the other (-k setA, ...).
"""
import pytest

import oracle
import scaled_cameras as sc
from DPE_MVS import _abi
from test_gpu_parity import assert_same, ctx  # noqa: F401  (ctx: the module-scoped context fixture)

pytestmark = pytest.mark.gpu


def _id(config, set_name, texel):
    return f"set{set_name[0]}-{config}-{set_name}-{texel}"


PAIRS = sc.pairs()
EXACT = [(c, s, t) for c, s, t in PAIRS if c in sc.PHOTOMETRIC and s in sc.EXACT_SETS]
_GPU = {}


def gpu_case(ctx, config, set_name, texel):
    """The device's outputs of a case, run once per module; its texel class is checked on the way."""
    key = (config, set_name, texel)
    if key not in _GPU:
        inp, st, _ = sc.case(config, set_name, texel)
        _GPU[key] = ctx.run(inp, st)
        assert ctx.last_stat(_abi.DPE_STAT_TEX_CLASS) == sc.TEXEL_CLASS[texel], key
    return _GPU[key]


@pytest.mark.parametrize("config,set_name,texel", PAIRS, ids=[_id(*p) for p in PAIRS])
def test_scaled_cameras_match_oracle(ctx, config, set_name, texel):
    want, _ = sc.oracle_case(config, set_name, texel)
    assert_same(gpu_case(ctx, config, set_name, texel), want, sc.case(config, set_name, texel)[2])


@pytest.mark.parametrize("config,set_name,texel", EXACT, ids=[_id(*p) for p in EXACT])
def test_exact_sets_match_the_unscaled_pass_on_the_device(ctx, config, set_name, texel):
    """A1 / A2 / A3 on the photometric passes: the slow (or negative) branch gives the device's own fast-branch
    bits.  Not for the geometric passes: world_point / project_cam take K[8] = 1."""
    assert_same(gpu_case(ctx, config, set_name, texel), gpu_case(ctx, config, None, texel),
                sc.case(config, set_name, texel)[2] + " vs unscaled, both on the device")


@pytest.mark.parametrize("set_name", ["A3_negative_small_plain", "C_dead_plain_overflow"],
                         ids=["setA-executes-A3_negative_small_plain", "setC-executes-C_dead_plain_overflow"])
def test_untimed_timed_and_counting_executes_scaled(ctx, set_name):
    """The three executes of test_gpu_parity.test_untimed_timed_and_counting_executes (two streams; one
    stream with events; one stream with counters) on a mixed and on a dead / overflowing case."""
    inp, st, what = sc.case("iter_80x60", set_name)
    want = oracle.run_pass(inp, st)
    ctx.stage(inp, st)
    try:
        ctx.execute()
        assert_same(ctx.fetch(), want, what + " untimed")
        ctx.set_timing(True)
        ctx.execute()
        assert_same(ctx.fetch(), want, what + " timed")
        ctx.set_timing(False)
        ctx.set_counting(True)
        ctx.execute()
        assert_same(ctx.fetch(), want, what + " counting")
    finally:
        ctx.set_timing(False)
        ctx.set_counting(False)
