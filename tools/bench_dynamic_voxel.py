"""Dev tool: ``DynamicVoxelizer`` next to the hard ``Voxelizer`` on the same synthetic batches -- the 0.075 m grid of
examples/active/bevfusion_lidar_*_spatial_temporal_feature.py, batch 4 and 32, device events around ``calls`` calls after
``warmup`` warm-up calls (each call includes its one small D2H); three windows per voxelizer, alternating, the median
reported.  Prints one JSON line per batch size: both times, the voxel counts, the dynamic workspace bytes and the hard
voxelizer's resident grid bytes.

  python tools/bench_dynamic_voxel.py [calls=20] [warmup=5]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from al3d import detector_ops as D, lib
from al3d.datasets import PoolFrames
from al3d.utils import Config

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")
hard_cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_lidar_spatial_temporal_feature.py")).voxel_generator
dyn_cfg = Config.fromfile(os.path.join(ROOT, "examples", "active",
                                       "bevfusion_lidar_dynamic_spatial_temporal_feature.py")).voxel_generator


def timed(fn):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls, out


for B in (4, 32):
    pool = PoolFrames.from_synthetic(B, dev, seed=7)
    pts = pool.flat
    off = torch.tensor(pool.offsets, dtype=torch.int64, device=dev)
    dyn = D.build_voxelizer(dyn_cfg, B, dev)
    hard = D.build_voxelizer(hard_cfg, B, dev)
    assert isinstance(dyn, D.DynamicVoxelizer) and isinstance(hard, D.Voxelizer)
    td, th = [], []
    for _ in range(3):                               # three windows each, alternating: the spread is part of the answer
        t, o_dyn = timed(lambda: dyn(pts, off))
        td.append(t)
        t, o_hard = timed(lambda: hard(pts, off))
        th.append(t)
    t_dyn, t_hard = sorted(td)[1], sorted(th)[1]
    print(json.dumps(dict(batch=B, points=int(pts.shape[0]), dynamic_ms=round(t_dyn, 3), hard_ms=round(t_hard, 3),
                          dynamic_ms_windows=[round(t, 3) for t in td], hard_ms_windows=[round(t, 3) for t in th],
                          dynamic_voxels=int(o_dyn["feat"].shape[0]), hard_voxels=int(o_hard["feat"].shape[0]),
                          dynamic_max_points_in_voxel=int(o_dyn["num_points"].max()),
                          dynamic_workspace_bytes=int(dyn.workspace_bytes(pts.shape[0], B)),
                          hard_workspace_bytes=int(lib.load().al3d_voxelize_workspace_bytes(pts.shape[0], B, hard.max_voxels)),
                          hard_grid_bytes=int(hard.grid.numel()))))
    del dyn, hard, o_dyn, o_hard
