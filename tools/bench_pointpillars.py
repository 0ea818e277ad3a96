"""Dev tool: frames/s of the PointPillars embedding sweep (examples/active/bevfusion_pointpillars_spatial_temporal_feature.py)
on the synthetic pool: voxelize with padded slots -> fused pillar net + scatter -> SECOND/SECONDFPN -> GAP, each
batch timed from the loader's voxelization to the embedding.  Also prints
the canvas bytes the scatter writes per batch and the peak device memory.

  python tools/bench_pointpillars.py [batch=32] [batches=6] [warmup=2]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from al3d import synthetic
from al3d.datasets import DeviceSweepLoader, PoolFrames
from al3d.models import build_detector
from al3d.utils import Config

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 6
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 2
dev = torch.device("cuda:0")
cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_pointpillars_spatial_temporal_feature.py"))
model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
synthetic.seeded_init_(model, seed=0)
model = model.to(dev).eval()
pool = PoolFrames.from_synthetic(B * (nb + warm), dev, seed=7)
loader = DeviceSweepLoader(pool, cfg.voxel_generator, None, batch_size=B, device=dev, with_points=True)
C = model.reader.out_channels
gx, gy = int(loader.voxelizer.grid_size[0]), int(loader.voxelizer.grid_size[1])
times, pillars = [], []
with torch.no_grad():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, ex in enumerate(loader):          # timed: the loader's voxelization (padded slots) + the model + GAP
        _, mid = model(ex, return_loss=False, estimate=True)
        emb = mid[-1].mean(-1).mean(-1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= warm:
            times.append(t1 - t0)
            pillars.append(int(ex["coordinates"].shape[0]))
        del mid, emb
        t0 = time.perf_counter()
times.sort()
med = times[len(times) // 2]
print(json.dumps(dict(batch=B, frames_per_s=round(B / med, 1), ms_per_batch=round(med * 1e3, 3),
                      pillars_per_batch=sum(pillars) // max(1, len(pillars)),
                      canvas_bytes=B * gy * gx * C * 4, pillar_row_bytes=sum(pillars) // max(1, len(pillars)) * C * 4,
                      peak_mem_gib=round(torch.cuda.max_memory_allocated(dev) / 2**30, 2))))
