"""Dev tool: the dynamic PointPillars reader against the hard one on one batch of the synthetic pool, per launch.

  hard:    Voxelizer (max_points_in_voxel 20, max_voxel_num 60000, padded slots)  +  al3d_pillar_net_scatter_f32
  dynamic: DynamicVoxelizer (no caps)                                             +  al3d_pillar_net_dynamic_f32 (canvas)

Both with the PointPillars example configs' geometry and [64, 64] filters.  Prints one JSON line: median microseconds per
call for the four pieces (the voxelizers include their one host sync), points and pillars per frame, the largest pillar,
and the atomic traffic of the dynamic net: ``atomic_bytes`` is what the pooling issues at most per call -- one 4-byte
integer max per output unit and per run of consecutive points of one pillar inside a 64-point wave chunk, both layers,
before the zero skip and the read test -- and ``atomic_bytes_per_s`` is that over the net's time.

  python tools/bench_pillar_dynamic.py [batch=8] [iters=20] [warmup=3]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from al3d import synthetic
from al3d.datasets import DeviceSweepLoader, PoolFrames
from al3d.detector_ops import build_voxelizer
from al3d.models import build_reader
from al3d.utils import Config

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 3
dev = torch.device("cuda:0")
act = os.path.join(ROOT, "examples", "active")
hard_cfg = Config.fromfile(os.path.join(act, "bevfusion_pointpillars_spatial_temporal_feature.py"))
dyn_cfg = Config.fromfile(os.path.join(act, "bevfusion_pointpillars_dynamic_spatial_temporal_feature.py"))
reader = build_reader(dict(dyn_cfg.model.reader))
synthetic.seeded_init_(reader, seed=0)
net = reader.to(dev).eval().net(dev)

pool = PoolFrames.from_synthetic(B, dev, seed=7)
ex = next(iter(DeviceSweepLoader(pool, dyn_cfg.voxel_generator, None, batch_size=B, device=dev, keep_points=True)))
pts, off = ex["points"], ex["point_offsets"]
hard_vox = build_voxelizer(hard_cfg.voxel_generator, B, dev)
dyn_vox = build_voxelizer(dyn_cfg.voxel_generator, B, dev)
nx, ny = int(dyn_vox.grid_size[0]), int(dyn_vox.grid_size[1])


def timed(fn):
    """Median microseconds of fn() over ``iters`` calls after ``warm``, by device events around each call."""
    out, us = None, []
    for i in range(warm + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        if i >= warm:
            us.append(a.elapsed_time(b) * 1e3)
    us.sort()
    return out, us[len(us) // 2]


with torch.no_grad():
    hv, hard_vox_us = timed(lambda: hard_vox(pts, off, want_voxels=True))
    _, hard_net_us = timed(lambda: net.canvas(hv["voxels"], hv["num_points"], hv["coords"], B, ny, nx))
    dv, dyn_vox_us = timed(lambda: dyn_vox(pts, off))
    _, dyn_net_us = timed(lambda: net.canvas_dynamic(pts, dv["point2voxel"], dv["feat"], dv["coords"], B, ny, nx,
                                                     check=False))
net.dynamic_status()

p2v = dv["point2voxel"].cpu()
idx = torch.arange(p2v.numel())
starts = torch.ones_like(p2v, dtype=torch.bool)
starts[1:] = p2v[1:] != p2v[:-1]
runs = int(((starts | (idx % 64 == 0)) & (p2v >= 0)).sum())
units = sum(p[3] for p in net.packs)
atomic_bytes = runs * units * 4
hard_us, dyn_us = hard_vox_us + hard_net_us, dyn_vox_us + dyn_net_us
print(json.dumps(dict(
    batch=B, hard_voxelize_us=round(hard_vox_us, 1), hard_net_scatter_us=round(hard_net_us, 1), hard_us=round(hard_us, 1),
    dynamic_voxelize_us=round(dyn_vox_us, 1), dynamic_net_us=round(dyn_net_us, 1), dynamic_us=round(dyn_us, 1),
    dynamic_over_hard=round(dyn_us / hard_us, 3), net_dynamic_over_hard=round(dyn_net_us / hard_net_us, 3),
    points_per_frame=int(pts.shape[0]) // B, in_range_points_per_frame=int((p2v >= 0).sum()) // B,
    hard_pillars_per_frame=int(hv["coords"].shape[0]) // B, dynamic_pillars_per_frame=int(dv["coords"].shape[0]) // B,
    largest_pillar=int(dv["num_points"].max()), pooled_runs=runs, atomic_bytes=atomic_bytes,
    atomic_bytes_per_s=round(atomic_bytes / (dyn_net_us * 1e-6), 1))))
