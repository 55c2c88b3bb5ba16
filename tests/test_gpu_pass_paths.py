"""GPU parity on the pass paths that the scenes of synthetic.make_scene never take (path_cases.py): the strong
sweep's edge scheme with more than 16 steps, steps longer than 2 pixels, the odd-length decrement and edge rays
used beyond 64 pixels (images of 2100 and 2880 px); the set-up chain with labels of -1 and foreign labels, no
STRONG pixel within 100 or none at all, all 64 support slots, windows of label 0 at the tiled limit and in the
untiled loop of k_gen_edge_inform, low-resolution walk indices out of range, column scans with carries.

tests/test_pass_paths.py asserts on the oracle alone that each input reaches those paths.  Here planes, weak,
sel and costs of every case must be the oracle's bit for bit.  One iteration (two on the two thinnest images),
three views.
"""
import pytest

import path_cases as pc
from DPE_MVS import _abi
from test_gpu_parity import assert_same, ctx  # noqa: F401  (ctx: the module-scoped context fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(pc.CASES))
def test_path_case_matches_oracle(ctx, name):
    inp, st, _ = pc.case(name)
    want, _ = pc.oracle_case(name)
    assert_same(ctx.run(inp, st), want, name)


@pytest.mark.parametrize("slots,over", [(0, None), (32, "gn_pts_gt32"), (8, "gn_pts_gt8")])
@pytest.mark.parametrize("name", ["full_slots_128x96", "lattice_96x64"])
def test_support_points_through_each_gen_neighbours_kernel(name, slots, over):
    """The 64-point case on k_gen_neighbours_lds<64> (0: rotate_time 4 takes 64 slots, nothing is deferred) and on
    the scratch kernel (32 / 8 slots: every pixel with more points is deferred, up to all 64 points each); the
    lattice case (rotate_time 2, at most 32 points) on k_gen_neighbours_lds<32> (0 and 32: none deferred) and with
    its pixels over 8 points on the scratch kernel.  The deferred count is the oracle's count of such pixels."""
    from DPE_MVS import native
    inp, st, _ = pc.case(name)
    want, stats = pc.oracle_case(name)
    assert stats["gn_pts_gt8"] > 0 and (name != "full_slots_128x96" or stats["gn_pts_eq64"] >= 16)
    c = native.PatchMatchContext(0)
    try:
        c.set_option(_abi.DPE_OPT_GN_SLOTS, slots)
        got = c.run(inp, st)
        deferred = c.last_stat(_abi.DPE_STAT_GN_DEFERRED)
    finally:
        c.close()
    assert deferred == (stats[over] if over else 0), (slots, deferred)
    assert_same(got, want, f"{name}, {slots} slots ({deferred} pixels deferred)")
