"""Census of the pass decisions (oracle.PATH_STATS) that the suite's inputs take, on the CPU oracle: the sum over
the older inputs (the 24 seeded random configurations of tests/test_gpu_parity.py, the configurations of
tests/test_gpu_setup_paths.py, 80x60x4 and 160x120x3 REFINE_ITER + geom) beside each case of tests/path_cases.py.
Prints the markdown table of DESIGN.md §4 ("pass paths").  No GPU needed.
Usage: python tools/path_census.py [--new-only]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("tests", "oracle", "dpe-mvs_amd"):
    sys.path.insert(0, os.path.join(ROOT, d))
import oracle  # noqa: E402
import path_cases as pc  # noqa: E402
import test_gpu_parity as tp  # noqa: E402
import test_gpu_setup_paths as ts  # noqa: E402
from DPE_MVS import synthetic  # noqa: E402


def add(total, st):
    for k, v in st.items():
        total[k] = max(total[k], v) if k in oracle.PATH_STATS_MAXIMA else total[k] + v


def older_inputs():
    for seed in range(24):
        W, H, N, kind, p = tp._random_case(seed)
        sc = synthetic.make_scene(W, H, N, seed=synthetic.SCENE_SEED + seed)
        st = synthetic.first_init_state(sc) if kind == "first" else synthetic.gt_state(sc, seed=seed)
        yield synthetic.pass_input(sc, p, depths=synthetic.src_depths(sc) if p.geom_consistency else None, seed=seed + 3), st
    for c in ts._CASES:
        kind, W, H, N, tex = c.values
        if tex != "u8":
            continue
        sc = synthetic.make_scene(W, H, N)
        yield synthetic.pass_input(sc, ts._params(kind), depths=synthetic.src_depths(sc), seed=W * 7 + N), \
            synthetic.gt_state(sc, seed=W + H)
    for W, H, N in ((80, 60, 4), (160, 120, 3)):
        yield pc.older_input(W, H, N, "refine_iter")


def main():
    cols = {}
    if "--new-only" not in sys.argv:
        total = dict.fromkeys(oracle.PATH_STATS, 0)
        n = 0
        for inp, st in older_inputs():
            oracle.run_pass(inp, st)
            add(total, oracle.last_path_stats())
            n += 1
        cols[f"older ({n})"] = total
    for name in pc.CASES:
        cols[name] = pc.oracle_case(name)[1]
    print("| count | " + " | ".join(cols) + " |")
    print("|---|" + "---:|" * len(cols))
    for k in oracle.PATH_STATS:
        print(f"| `{k}` | " + " | ".join(str(c[k]) for c in cols.values()) + " |")


if __name__ == "__main__":
    main()
