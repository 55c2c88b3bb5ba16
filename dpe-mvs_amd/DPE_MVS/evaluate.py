"""python -m DPE_MVS.evaluate recon.ply gt.ply --tau T [T ...] [--radius R] [--voxel V] [--crop x0 y0 z0 x1 y1 z1]
                              [--gpu N | --cpu] [--json FILE] [--register R [R ...]] [--register-iters N]
                              [--register-init T0 .. T11]

Precision, recall and F-score of a reconstructed PLY (DPE/DPE.ply of a run with fusion) against a
ground-truth PLY: pipeline.evaluate_clouds over the two files, the table and numbers of bin/dpe_eval.  Without
--gpu the distances run on host threads; with it on that device: the same numbers.  The clouds are taken as
they are unless --crop keeps the points inside a box and --voxel down-samples both clouds to one point per voxel
first (pipeline.evaluate_clouds' crop and voxel), and --register first moves the reconstruction onto the ground
truth by point-to-point ICP over 1 to 4 radii, coarse to fine (pipeline.evaluate_clouds' register).
"""
from __future__ import annotations

import argparse
import json
import sys

from . import pipeline


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m DPE_MVS.evaluate", description=__doc__.split("\n\n")[1])
    ap.add_argument("recon")
    ap.add_argument("gt")
    ap.add_argument("--tau", type=float, nargs="+", required=True, help="distance thresholds (1 to 16)")
    ap.add_argument("--radius", type=float, default=None, help="truncation radius (default: the largest tau)")
    ap.add_argument("--gpu", type=int, default=-1, help="device of the distances (default: host threads)")
    ap.add_argument("--cpu", action="store_true", help="host threads (the default)")
    ap.add_argument("--voxel", type=float, default=None, help="down-sample both clouds to one point per voxel of this edge first")
    ap.add_argument("--crop", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="keep the points of both clouds inside this box first")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--register", type=float, nargs="+", default=None, metavar="R",
                    help="register the reconstruction to the ground truth first: 1 to 4 match radii, coarse to fine")
    ap.add_argument("--register-iters", type=int, default=50, help="steps per radius at most (default 50)")
    ap.add_argument("--register-init", type=float, nargs=12, default=None, metavar="T", help="starting transform, 3 rows of 4")
    a = ap.parse_args(argv)
    try:
        crop = None if a.crop is None else (a.crop[:3], a.crop[3:])
        register = None if a.register is None else dict(radii=a.register, max_iters=a.register_iters, init=a.register_init)
        e = pipeline.evaluate_clouds(pipeline.read_point_cloud(a.recon), pipeline.read_point_cloud(a.gt), a.tau, a.radius,
                                     -1 if a.cpu else a.gpu, voxel=a.voxel, crop=crop, register=register)
    except pipeline.PipelineError as err:
        print(f"evaluate: {err}", file=sys.stderr)
        return 1
    sys.stdout.write(pipeline.format_cloud_eval(e))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(e, n_tau=len(e["tau"])), f)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
