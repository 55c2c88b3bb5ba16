"""python -m DPE_MVS.voxel in.ply out.ply V [--gpu N | --cpu]

Thins a PLY to one point per voxel of edge V and keeps its colours (pipeline.voxel_down_sample; include/dpe_mvs.h,
dpe_cloud_voxel, states what a voxel's point is), what bin/dpe_voxel does: the same bytes.  Without --gpu the serial
host loop runs; with it that device: the same points.  The point counts before and after go to stderr.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import pipeline


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m DPE_MVS.voxel", description=__doc__.split("\n\n")[1])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("voxel", type=float)
    ap.add_argument("--gpu", type=int, default=-1, help="device (default: the host loop)")
    ap.add_argument("--cpu", action="store_true", help="the host loop (the default)")
    a = ap.parse_args(argv)
    try:
        xyz, rgb = pipeline.read_point_cloud_colors(a.input)
        out, col, _, _ = pipeline.voxel_down_sample(xyz, a.voxel, rgb, -1 if a.cpu else a.gpu)
        pts = np.zeros((len(out), 6), np.float32)
        pts[:, :3] = out
        if col is not None:
            pts[:, 3:] = col
        pipeline.write_point_cloud(a.output, pts)
    except (pipeline.PipelineError, RuntimeError) as err:
        print(f"voxel: {err}", file=sys.stderr)
        return 1
    print("voxel: %d points -> %d points (voxel %.9g)" % (len(xyz), len(out), np.float32(a.voxel)), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
