"""Python launcher with the positional arguments of the reference's `DPE` binary (main.cpp:602-635);
the native command line is dpe-mvs_amd/bin/dpe (same arguments, RCCL across ranks):

    python -m DPE_MVS dense_folder [gpu_index] [verbose] [viz] [fusion] [depth] [normal] [weak] [edge] [point_cloud]

point_cloud (an addition: the reference's call is commented out, main.cpp:456-466): off (0, the default),
all (1) or strong (2) writes point_<it>.ply per image after the last pass of every resolution round.

Multi-GPU (one process per GPU, reference images sharded, depth maps all-gathered over RCCL):

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m DPE_MVS dense_folder
"""
from __future__ import annotations

import os
import sys

USAGE = ("USAGE: DPE dense_folder [gpu_index] [verbose] [viz] [fusion] [depth] [normal] [weak] [edge]"
         " [point_cloud: off | all | strong]")
_POINT_CLOUD = {"0": 0, "off": 0, "1": 1, "all": 1, "2": 2, "strong": 2}


def main(argv: list) -> int:
    if len(argv) < 2:
        print(USAGE, file=sys.stderr)
        return 1
    point_cloud = 0
    if len(argv) > 10:
        if argv[10] not in _POINT_CLOUD:
            print(f"bad point_cloud {argv[10]!r}\n{USAGE}", file=sys.stderr)
            return 1
        point_cloud = _POINT_CLOUD[argv[10]]
    a = [int(x) for x in argv[2:10]]
    opt = lambda i, d: a[i] if len(a) > i else d
    gpu_index, verbose, viz, fusion = opt(0, 0), bool(opt(1, 1)), bool(opt(2, 0)), bool(opt(3, 0))
    depth, normal, weak, edge = bool(opt(4, 1)), bool(opt(5, 0)), bool(opt(6, 0)), bool(opt(7, 0))
    from . import pipeline
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        try:
            return pipeline.run_dpe_pipeline(argv[1], local, verbose, fusion, viz, depth, normal, weak, edge, dist=dist,
                                             point_cloud=point_cloud)
        finally:
            dist.destroy_process_group()
    if point_cloud:   # DPE_MVS.dpe_mvs keeps the reference binding's parameters: the option goes through the C++ pipeline's ctypes entry
        return pipeline.run_dpe_pipeline(argv[1], gpu_index, verbose, fusion, viz, depth, normal, weak, edge, point_cloud=point_cloud)
    return pipeline.dpe_mvs(argv[1], gpu_index, verbose, fusion, viz, depth, normal, weak, edge)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
