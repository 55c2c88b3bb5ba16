"""The decisions one pass takes, counted on the oracle (oracle.PATH_STATS): every input of path_cases.py must
reach the paths it was built for, and the cases together with four of the suite's older inputs must reach every
counted path but the ones named, with the reason, in UNREACHED.  tests/test_gpu_pass_paths.py then compares
the device with the oracle on the same inputs; a parity test proves nothing about a branch no input takes.

Floors: a tenth of the count the case showed when it was designed (the issue's table), else > 0.  No case may be
vacuous: at least half of its output pixels (a quarter on the thin 2100 / 2880 px images, whose cameras see
little of the scene) end with a photometric cost below 2, i.e. with a plane that matches some view.
"""
import pytest

import oracle
import path_cases as pc
from golden_io import bits_equal

STEP_NUM = [f"ps_step_num_{n}" for n in range(11, 23)]

# name -> why no input the reference can produce takes the path
UNREACHED = {
    "ps_len3_c": "the parity rule itself: for d < 4 an odd step_len is decremented (DPE.cu:1263), so after it "
                 "step_len is even and the bin 3 cannot hold a scan; the bin exists to show exactly that",
    "pw_slot_not_strong": "a neighbour slot is written by GenNeighbours from strong_points[], which holds only pixels "
                          "that are STRONG (the probe's own test, or FindNearestStrongPoint's), and the weak map changes "
                          "before the weak sweep only in NeigbourUpdate, WEAK -> UNKNOWN: a slot never names a pixel "
                          "that is not STRONG, whatever the input maps are",
    "d2w_od_zero": "DepthToWeak reads the depth GetDepthandNormal wrote: a plane enters a pass from depths.dmb (written "
                   "by the reference, DPE.cpp:887-903; RescaleMatToTargetSize interpolates) or from a draw inside "
                   "[depth_min, depth_max], and a sweep, the refinement or LocalRefine replaces it only by a depth in that "
                   "range with depth_min > 0; the median of FilterStrong picks or averages such depths.  A zero depth "
                   "needs a depths.dmb the reference never writes",
}


def _share(out):
    return float((out["costs"] < 2.0).mean())


def _check(name, floors, share):
    out, st = pc.oracle_case(name)
    print(name, {k: st[k] for k in floors}, "cost < 2 share", round(_share(out), 3))
    for k, lo in floors.items():
        assert st[k] >= lo, (name, k, st[k], lo)
    assert _share(out) >= share, (name, _share(out))
    return st


def test_names_match_the_library():
    assert oracle.path_stat_names() == oracle.PATH_STATS
    assert set(oracle.PATH_STATS_MAXIMA) <= set(oracle.PATH_STATS)
    assert len(UNREACHED) <= 3 and set(UNREACHED) <= set(oracle.PATH_STATS)


def test_counts_do_not_depend_on_threads_and_reset():
    inp, st = pc.older_input(*pc.OLDER["iter_80x60"])
    a = oracle.run_pass(inp, st, threads=1)
    sa = oracle.last_path_stats()
    b = oracle.run_pass(inp, st, threads=5)
    sb = oracle.last_path_stats()
    assert sa == sb
    for k in a:
        assert bits_equal(a[k], b[k]), k
    assert sa["ps_scans"] > 0
    assert sa["ps_scans"] == sa["ps_centre_on_edge"] + sa["ps_ray_clipped"] + sa["ps_ray_used"] == sum(sa[k] for k in STEP_NUM)
    assert sa["gn_weak"] == sa["gn_edge_limit_on"] + sa["gn_edge_limit_off"]


def test_older_inputs_reach_the_fit_branches_and_not_the_new_paths():
    """What the census of the suite's inputs showed: the GenNeighbours / RANSAC branches are taken,
    the edge scheme has one shape of scan, labels are never -1, some STRONG pixel is always near."""
    _, st = pc.oracle_older("iter_80x60")
    for k in ("walk_blocked", "gn_ext_foreign_drop", "gn_degenerate", "gn_inliers_lt6", "gn_tie_won", "gn_thr_tightened",
              "gn_thr_kept", "gn_pair_block", "gn_triangle_optional", "gn_no_plane"):
        assert st[k] > 0, k
    assert st["ps_step_num_11"] == st["ps_scans"] > 0 and st["ps_len2_c"] + st["ps_len2_d"] == st["ps_scans"]
    for k in ("ps_odd_decrement", "ps_ray_used_ge64", "gei_ray_stop_minus1", "gei_window_all_label0", "fns_none",
              "gn_probe_none", "gn_ext_none", "walk_lowres_oob", "gn_pts_eq64"):
        assert st[k] == 0, k
    assert 0 < st["fns_max_radius"] < 64


def test_thin_2100x16():
    st = pc.oracle_case("thin_2100x16")[1]
    assert sum(st[k] for k in STEP_NUM[1:]) >= 53165        # step_num > 11
    assert sum(st[k] for k in STEP_NUM[6:]) >= 53037        # step_num > 16: the third batch of 8 loads
    _check("thin_2100x16", {"ps_odd_decrement": 25991}, 0.25)


def test_thin_2880x14():
    st = _check("thin_2880x14", {"ps_len4_c": 1, "ps_len3_d": 1}, 0.25)
    assert st["ps_len3_c"] + st["ps_len4_c"] + st["ps_len3_d"] + st["ps_len4_d"] >= 63297      # step_len > 2
    assert st["ps_len3_d"] + st["ps_len4_d"] >= 32066


def test_wide_2100x96():
    _check("wide_2100x96", {"ps_lengt2_used_d": 240}, 0.25)


def test_edge_lines_2880x96():
    floors = dict.fromkeys(STEP_NUM, 1)
    # step_len 2, 3 and >= 4 for d >= 4, 2 and >= 4 for d < 4; longer than 2 with the ray used, and clipped rays
    floors.update(dict.fromkeys(["ps_len2_c", "ps_len4_c", "ps_len2_d", "ps_len3_d", "ps_len4_d", "ps_odd_decrement",
                                 "ps_lengt2_used_c", "ps_lengt2_used_d", "ps_ray_clipped", "ps_ray_used_ge64",
                                 "ps_centre_on_edge", "ps_second_no_first", "ps_second_more_good", "ps_second_fewer_bad"], 1))
    st = _check("edge_lines_2880x96", floors, 0.25)
    assert st["ps_len4_c"] + st["ps_len3_d"] + st["ps_len4_d"] > st["ps_lengt2_used_c"] + st["ps_lengt2_used_d"]   # clipped ones


def test_tall_40x150():
    # rings and column scans longer than one 64-lane step; rows 0 / 149 hold several STRONG pixels of a ring
    _check("tall_40x150", {"fns_max_radius": 64, "fns_ring_multi": 1, "ps_ray_used": 1, "gn_pts_le3": 1, "gn_weak": 1}, 0.5)


def test_one_column_230x40():
    st = _check("one_column_230x40", {"gn_probe_none": 96148, "walk_lowres_oob": 499, "gn_pts_le3": 579,
                                      "gn_ext_none": 1, "fns_ring_multi": 1}, 0.5)
    assert st["fns_max_radius"] == 100
    assert st["fns_found_r100"] == 40           # x = 108, every row
    assert st["fns_none"] == 40 * (230 - 109)   # x >= 109


def test_all_weak_48x32():
    st = _check("all_weak_48x32", {"gn_probe_none": 1}, 0.5)
    assert st["gn_probe_none"] == st["gn_probe_nearest"]
    assert st["fns_none"] == st["gn_weak"] == st["gn_pts_le3"] == 48 * 32
    assert st["fit_none"] + st["fit_found"] + st["pw_slot_used"] + st["pw_slot_none"] == 0    # every pixel UNKNOWN: no weak sweep


def test_lattice_96x64():
    _check("lattice_96x64", {"gei_ray_stop_minus1": 361, "gn_ext_foreign_drop": 230, "gei_ray_past_foreign": 1,
                             "gei_ray_len_gt16": 1, "gn_normal_skip": 1}, 0.5)


def test_full_slots_128x96():
    _check("full_slots_128x96", {"gn_pts_gt32": 14, "gn_pts_eq64": 16}, 0.5)


@pytest.mark.parametrize("name", ["label0_block_r5", "label0_block_r8", "label0_block_r9"])
def test_label0_block(name):
    _check(name, {"gei_window_all_label0": 1, "gn_edge_limit_off": 1, "gn_edge_limit_on": 1}, 0.5)


def test_every_counted_path_is_reached():
    total = dict.fromkeys(oracle.PATH_STATS, 0)
    for st in [pc.oracle_case(n)[1] for n in pc.CASES] + [pc.oracle_older(n)[1] for n in pc.OLDER]:
        for k, v in st.items():
            total[k] = max(total[k], v) if k in oracle.PATH_STATS_MAXIMA else total[k] + v
    print(total)
    missing = sorted(k for k, v in total.items() if v == 0)
    assert missing == sorted(UNREACHED), missing
