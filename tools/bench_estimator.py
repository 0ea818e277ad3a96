"""Dev tool: what the box-wise IoU estimator costs beside the sweep it rides on, at the CBGS shape.

One batch of ``frames`` synthetic frames (ten-sweep clouds) through the CBGS detector (examples/active/estimator/
cbgs_partial.py, seeded weights, seeded estimator); its own 6 x 83 NMS slots and the batch's points are the estimator's input.

* ``estimate_us``: ``selector_ops.estimate_boxes(check=False)`` -- the two memsets and the three launches (prep, points,
  head) -- device events around ``calls`` calls after ``warmup`` warm-up calls; three windows, the median reported.  The
  split by kernel comes from a run of its own under ``rocprofv3 --kernel-trace --stats`` (kernels est_prep_kernel,
  est_points_kernel, est_head_kernel).
* ``pairs``: points x valid boxes summed over the frames, the membership tests the brute-force pass makes; ``hits``: the
  (point, box) pairs that pass, i.e. runs of the point network; ``survivors``: boxes that keep a point.
* ``rescored_sweep_ms`` / ``plain_sweep_ms``: ``sweep_embeddings(with_entropy=True)`` over a pool of ``frames`` frames in
  batches of 8 through ``WithEstimator`` and through the detector alone, wall clock around a synchronised call,
  alternating, the median of three.

  python tools/bench_estimator.py [frames=128] [calls=20] [warmup=5]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from al3d import selector_ops as ops, synthetic
from al3d.datasets import DeviceSweepLoader, PoolFrames, generate_task_anchors
from al3d.models import WithEstimator, build_detector, build_estimator
from al3d.sweep import sweep_embeddings
from al3d.utils import Config

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 128
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "estimator", "cbgs_partial.py"))
model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
synthetic.seeded_init_(model, seed=0)
model = model.to(dev).eval()
est = build_estimator(cfg.estimator)
synthetic.seeded_init_(est, seed=5)
est = est.to(dev).eval()
anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])
pool = PoolFrames.from_synthetic(frames, dev, num_base=4, seed=3)

with torch.no_grad():
    batch = next(iter(DeviceSweepLoader(pool, cfg.voxel_generator, anchors, frames, device=dev, keep_points=True)))
    preds, _ = model(batch, return_loss=False, estimate=True)
boxes, scores, labels, counts, done, meta = preds._raw
torch.cuda.current_stream().wait_event(done)
points, off = batch["points"].contiguous(), batch["point_offsets"].to(torch.int64)
wts = est.packed_weights(dev)
out = None


def call():
    global out
    out = ops.estimate_boxes(boxes, labels, counts, points, off, wts, est.num_classes, check=False)


win = []
for _ in range(3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        call()
    b.record()
    torch.cuda.synchronize()
    win.append(a.elapsed_time(b) / calls * 1000.0)
ops.estimator_status_check(out["status"].item())
valid = counts.clamp(0, boxes.shape[2]).sum(dim=1).to(torch.int64)
pairs = int(((off[1:] - off[:-1]) * valid).sum())


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000.0


plain = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, 8, device=dev)
kept = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, 8, device=dev, keep_points=True)
both = WithEstimator(model, est)
wall(lambda: sweep_embeddings(model, plain, dev, num_frames=frames, with_entropy=True))     # warm-up of both paths
wall(lambda: sweep_embeddings(both, kept, dev, num_frames=frames, with_entropy=True))
tp, tr = [], []
for _ in range(3):
    tp.append(wall(lambda: sweep_embeddings(model, plain, dev, num_frames=frames, with_entropy=True)))
    tr.append(wall(lambda: sweep_embeddings(both, kept, dev, num_frames=frames, with_entropy=True)))
print(json.dumps(dict(frames=frames, slots_per_frame=boxes.shape[1] * boxes.shape[2], points=int(points.shape[0]),
                      boxes_per_frame=float(valid.sum()) / frames, pairs=pairs, hits=int(out["npts"].sum()),
                      survivors=int(out["counts"].sum()), estimate_us=round(sorted(win)[1], 1),
                      estimate_us_windows=[round(t, 1) for t in win],
                      rescored_sweep_ms=round(sorted(tr)[1], 1), rescored_sweep_ms_windows=[round(t, 1) for t in tr],
                      plain_sweep_ms=round(sorted(tp)[1], 1), plain_sweep_ms_windows=[round(t, 1) for t in tp])))
