"""python -m DPE_MVS.register src.ply tgt.ply out.ply R [R ...] [--iters N] [--init T0 .. T11] [--gpu N | --cpu]

Moves a source PLY onto a target PLY by point-to-point ICP over 1 to 4 match radii, coarse to fine
(pipeline.register_clouds; include/dpe_host.h, dpe_host_cloud_register, states the loop) and writes the source
transformed with its colours kept, what bin/dpe_register does: the same bytes.  Without --gpu the host step runs;
with it that device: the same transform.  Prints T and one line per stage.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import pipeline


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m DPE_MVS.register", description=__doc__.split("\n\n")[1])
    ap.add_argument("source")
    ap.add_argument("target")
    ap.add_argument("output")
    ap.add_argument("radii", type=float, nargs="+", help="1 to 4 match radii, coarse to fine")
    ap.add_argument("--iters", type=int, default=50, help="steps per radius at most (default 50)")
    ap.add_argument("--init", type=float, nargs=12, default=None, metavar="T", help="starting transform, 3 rows of 4")
    ap.add_argument("--gpu", type=int, default=-1, help="device (default: the host step)")
    ap.add_argument("--cpu", action="store_true", help="the host step (the default)")
    a = ap.parse_args(argv)
    try:
        xyz, rgb = pipeline.read_point_cloud_colors(a.source)
        reg = pipeline.register_clouds(xyz, pipeline.read_point_cloud(a.target), a.radii, max_iters=a.iters, init=a.init,
                                       gpu_index=-1 if a.cpu else a.gpu)
        pts = np.zeros((len(xyz), 6), np.float32)
        pts[:, :3] = pipeline.transform_cloud(reg["T"], xyz)
        if rgb is not None:
            pts[:, 3:] = rgb
        pipeline.write_point_cloud(a.output, pts)
    except (pipeline.PipelineError, RuntimeError) as err:
        print(f"register: {err}", file=sys.stderr)
        return 1
    sys.stdout.write(format_registration(reg, len(xyz)))
    return 0


def format_registration(reg: dict, n: int) -> str:
    """What bin/dpe_register prints, from register_clouds' dict."""
    rows = ["T %.17g %.17g %.17g %.17g" % tuple(row) for row in reg["T"]]
    rows += ["stage %d: radius %.9g, %d steps, %d of %d matched, rms %.9g, converged %d"
             % (k, s["radius"], s["iters"], s["matched"], n, s["rms"], s["converged"]) for k, s in enumerate(reg["stages"])]
    return "\n".join(rows) + "\n"


if __name__ == "__main__":
    sys.exit(main())
