"""Dev tool: what the PPAL / CALD pre-pass matching costs beside the sweep it rides on.

One batch of ``frames`` synthetic frames through the CBGS detector (examples/active/cbgs_cald.py, seeded weights); its own
detections are the reference boxes (CALD's shape: up to 498 boxes on both sides of every frame).

* ``match_us``: ``LazyDetections.match`` on the raw NMS buffers -- device events around ``calls`` calls after ``warmup``
  warm-up calls, each call with its memsets, the launch and the one status read-back; three windows, the median reported.
* ``host_ms``: the route the reference takes on the same batch: materialise the per-frame dictionaries (device -> host)
  and run the numpy restatement of the loop (tests/prepass_numpy.py).  The loop is timed on the first ``host_frames``
  frames and scaled to the batch (``host_ms_scaled``); the materialisation is timed on the whole batch.
* ``prepass_sweep_ms`` / ``plain_sweep_ms``: one ``sweep_matches`` over a pool of ``frames`` frames in batches of 8 against
  one ``sweep_embeddings(with_entropy=True)`` over the same loader, wall clock around a synchronised call, alternating,
  the median of three.  The pre-pass loop is the serial one of ``PPALSelector.buffer_pred``; the plain sweep is pipelined
  over two streams, so the pair compares the two entry points as they are, not the matching alone.

  python tools/bench_prepass.py [frames=128] [calls=20] [warmup=5] [host_frames=4]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

from al3d import synthetic
from al3d.datasets import DeviceSweepLoader, PoolFrames, generate_task_anchors
from al3d.models import build_detector
from al3d.selectors import prepass as P
from al3d.sweep import sweep_embeddings
from al3d.utils import Config

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 128
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
host_frames = int(sys.argv[4]) if len(sys.argv) > 4 else 4
dev = torch.device("cuda:0")
cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "cbgs_cald.py"))
model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
synthetic.seeded_init_(model, seed=0)
model = model.to(dev).eval()
anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])
pool = PoolFrames.from_synthetic(frames, dev, num_base=4, seed=3)
ncls = len(P.head_class_names(model))

with torch.no_grad():
    batch = next(iter(DeviceSweepLoader(pool, cfg.voxel_generator, anchors, frames, device=dev)))
    preds, _ = model(batch, return_loss=False, estimate=True)
boxes, scores, labels, counts = P._raw_of(preds)
torch.cuda.synchronize()
refs = P.FrameRefs.from_frames(frames, {
    b: (torch.cat([boxes[b, t, :int(c)] for t, c in enumerate(counts[b].tolist())]).cpu().numpy(),
        torch.cat([labels[b, t, :int(c)] for t, c in enumerate(counts[b].tolist())]).cpu().numpy(),
        torch.cat([scores[b, t, :int(c)] for t, c in enumerate(counts[b].tolist())]).cpu().numpy())
    for b in range(frames)})
dev_refs = refs.batch(list(range(frames)), dev)


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


win = []
for _ in range(3):
    t, out = timed(lambda: preds.match(dev_refs, ncls=ncls))
    win.append(t * 1000.0)
matches = int(out["cls_count"].sum())

# the host route
t0 = time.perf_counter()
preds._list = None
dicts = list(preds)
host = [(d["box3d_lidar"].cpu().numpy(), d["scores"].cpu().numpy(), d["label_preds"].cpu().numpy()) for d in dicts]
t_mat = (time.perf_counter() - t0) * 1000.0
import prepass_numpy as PN  # noqa: E402

hb, hs, hl, hc = (t[:host_frames].cpu().numpy() for t in (boxes, scores, labels, counts))
t0 = time.perf_counter()
PN.match_frames(hb, hs, hl, hc, refs.boxes, refs.labels, refs.scores, refs.off[:host_frames + 1], ncls)
t_loop = (time.perf_counter() - t0) * 1000.0

# the sweeps
loader = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, 8, device=dev)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000.0


wall(lambda: sweep_embeddings(model, loader, dev, num_frames=frames, with_entropy=True))      # warm-up of both paths
wall(lambda: P.sweep_matches(model, loader, dev, refs, ncls=ncls))
tp, ts = [], []
for _ in range(3):
    ts.append(wall(lambda: sweep_embeddings(model, loader, dev, num_frames=frames, with_entropy=True)))
    tp.append(wall(lambda: P.sweep_matches(model, loader, dev, refs, ncls=ncls)))
print(json.dumps(dict(frames=frames, boxes_per_frame=float(counts.sum().item()) / frames, matches=matches,
                      match_us=round(sorted(win)[1], 1), match_us_windows=[round(t, 1) for t in win],
                      materialise_ms=round(t_mat, 2), host_loop_frames=host_frames, host_loop_ms=round(t_loop, 1),
                      host_ms_scaled=round(t_mat + t_loop * frames / host_frames, 1),
                      prepass_sweep_ms=round(sorted(tp)[1], 1), prepass_sweep_ms_windows=[round(t, 1) for t in tp],
                      plain_sweep_ms=round(sorted(ts)[1], 1), plain_sweep_ms_windows=[round(t, 1) for t in ts])))
