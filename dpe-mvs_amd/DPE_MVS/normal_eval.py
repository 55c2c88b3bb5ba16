"""python -m DPE_MVS.normal_eval dense_folder gt.ply radius tau_deg [tau_deg ...] [--splat S] [--min-neighbours N] [--maps]
                                 [--json FILE] [--gpu N | --cpu]
   python -m DPE_MVS.normal_eval dense_folder tau_deg [tau_deg ...] --gt-normals DIR [...]

The normal maps DPE/%08d/normal.npy of a dense folder against the normals of a ground-truth scan, estimated per point by
PCA over the points within `radius` and rendered into each view beside the z-buffer, or against ground-truth normal
maps: pipeline.evaluate_normal_maps, the table and numbers of bin/dpe_normal_eval.  Without --gpu everything runs on
the host; with it on that device: the same numbers.  A row per image in ascending id and a total: the pixels where the
ground truth, the estimate and both hold a normal, the mean cosine distance, the median and mean angle in degrees
(from a 1 degree histogram) over the latter, and per threshold the share within the angle (within / both) and the
completeness (within / ground truth).
"""
from __future__ import annotations

import argparse
import json
import sys

from . import pipeline


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m DPE_MVS.normal_eval", description=__doc__.split("\n\n")[1])
    ap.add_argument("dense_folder")
    ap.add_argument("rest", nargs="+", metavar="gt.ply radius tau_deg [tau_deg ...]",
                    help="the scan and the PCA radius (both left out with --gt-normals), then 1 to 16 angles in degrees")
    ap.add_argument("--splat", type=int, default=0, help="half-width of a scan point's footprint in pixels, 0 to 8 (default 0)")
    ap.add_argument("--min-neighbours", type=int, default=3, help="points within the radius a normal needs, itself included, 3 at least (default 3)")
    ap.add_argument("--gt-normals", default=None, metavar="DIR", help="DIR/%%08d.npy [h][w][3] are the ground truth instead of a scan")
    ap.add_argument("--maps", action="store_true", help="write normal_gt.npy and normal_error.npy beside each map")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--gpu", type=int, default=-1, help="device of the normals, the render and the score (default: the host)")
    ap.add_argument("--cpu", action="store_true", help="the host (the default)")
    a = ap.parse_args(argv)
    try:
        nums = [float(v) for v in (a.rest if a.gt_normals is not None else a.rest[1:])]
    except ValueError:
        ap.error("a radius or a threshold is not a number")
    radius, taus = (None, nums) if a.gt_normals is not None else (nums[0] if nums else None, nums[1:])
    if not taus:
        ap.error("at least one threshold expected")
    try:
        gt = None if a.gt_normals is not None else pipeline.read_point_cloud(a.rest[0])
        e = pipeline.evaluate_normal_maps(a.dense_folder, gt, radius, taus, min_neighbours=a.min_neighbours, splat=a.splat,
                                          gt_normals=a.gt_normals, write_maps=a.maps, gpu_index=-1 if a.cpu else a.gpu)
    except pipeline.PipelineError as err:
        print(f"normal_eval: {err}", file=sys.stderr)
        return 1
    sys.stdout.write(pipeline.format_normal_eval(e))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(e, f)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
