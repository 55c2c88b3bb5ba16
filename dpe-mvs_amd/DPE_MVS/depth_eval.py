"""python -m DPE_MVS.depth_eval dense_folder gt.ply tau [tau ...] [--relative] [--splat S] [--map NAME.npy] [--maps]
                                [--json FILE] [--gpu N | --cpu]
   python -m DPE_MVS.depth_eval dense_folder tau [tau ...] --gt-maps DIR [...]

The depth maps DPE/%08d/depth.npy of a dense folder against a ground-truth scan rendered into each view with a
z-buffer, or against ground-truth maps: pipeline.evaluate_depth_maps, the table and numbers of bin/dpe_depth_eval.
Without --gpu the render and the score run on the host; with it on that device: the same numbers.  A row per
image in ascending id and a total: the usable pixels of the ground truth, of the estimate and of both, the mean
absolute and relative error and the RMSE over the latter, and per threshold the accuracy (within / both) and the
completeness (within / ground truth).
"""
from __future__ import annotations

import argparse
import json
import sys

from . import pipeline


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m DPE_MVS.depth_eval", description=__doc__.split("\n\n")[1])
    ap.add_argument("dense_folder")
    ap.add_argument("rest", nargs="+", metavar="gt.ply tau [tau ...]", help="the scan (left out with --gt-maps), then 1 to 16 thresholds")
    ap.add_argument("--relative", action="store_true", help="|est - gt| < tau * gt instead of < tau")
    ap.add_argument("--splat", type=int, default=0, help="half-width of a scan point's footprint in pixels, 0 to 8 (default 0)")
    ap.add_argument("--map", default="depth.npy", help="the map to score: depth.npy (the default) or depth_filtered.npy")
    ap.add_argument("--gt-maps", default=None, metavar="DIR", help="DIR/%%08d.npy are the ground truth instead of a scan")
    ap.add_argument("--maps", action="store_true", help="write depth_gt.npy and depth_error.npy beside each map")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--gpu", type=int, default=-1, help="device of the render and the score (default: the host)")
    ap.add_argument("--cpu", action="store_true", help="the host (the default)")
    a = ap.parse_args(argv)
    try:
        taus = [float(v) for v in (a.rest if a.gt_maps is not None else a.rest[1:])]
    except ValueError:
        ap.error("a threshold is not a number")
    if not taus:
        ap.error("at least one threshold expected")
    try:
        gt = None if a.gt_maps is not None else pipeline.read_point_cloud(a.rest[0])
        e = pipeline.evaluate_depth_maps(a.dense_folder, gt, taus, relative=a.relative, splat=a.splat, map_name=a.map,
                                         gt_maps=a.gt_maps, write_maps=a.maps, gpu_index=-1 if a.cpu else a.gpu)
    except pipeline.PipelineError as err:
        print(f"depth_eval: {err}", file=sys.stderr)
        return 1
    sys.stdout.write(pipeline.format_depth_eval(e))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(e, f)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
