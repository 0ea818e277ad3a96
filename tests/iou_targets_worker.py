"""Worker of tests/test_box_iou_consumers_gpu.py -- launched by ``python -m torch.distributed.run`` with two gloo ranks that
share cuda:0 (the style of tests/dist_sweep_worker.py).  Each rank runs ``sweep_iou_targets`` over its contiguous shard of a
planted five-frame pool (3 + 2 frames, one frame without a detection, one without ground truth) with a stub detector that
hands back planted per-frame boxes; the gathered rows must be, in dataset order, what ``box_iou_best`` gives on the whole
pool in one call."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_FRAMES = 5


def planted_pool(seed=31):
    """-> (per-frame detections [(boxes [k,9], scores [k], labels [k])], ground truth {frame: (boxes [m,9], labels, scores)})"""
    rng = np.random.default_rng(seed)

    def boxes(k, around=None):
        b = np.zeros((k, 9), np.float32)
        b[:, :2] = rng.uniform(-20, 20, (k, 2)) if around is None else around[:k, :2] + rng.uniform(-0.7, 0.7, (k, 2))
        b[:, 2] = rng.uniform(-1.5, -0.5, k)
        b[:, 3:6] = np.array([1.97, 4.63, 1.7]) * rng.uniform(0.8, 1.2, (k, 3))
        b[:, 6:8] = rng.uniform(-3, 3, (k, 2))
        b[:, 8] = rng.uniform(-np.pi, np.pi, k) if around is None else around[:k, 8] + rng.uniform(-0.2, 0.2, k)
        return b
    gt, dets = {}, []
    for i, (m, k) in enumerate(((6, 4), (3, 0), (0, 3), (5, 5), (2, 2))):
        g = boxes(m)
        gt[i] = (g, rng.integers(0, 3, m).astype(np.int32), np.full(m, -1.0, np.float32))
        d = boxes(k, around=g) if m >= k and m else boxes(k)
        dets.append((d, rng.uniform(0.1, 0.9, k).astype(np.float32), rng.integers(0, 3, k).astype(np.int64)))
    return dets, gt


class PlantedDetector(torch.nn.Module):
    """detector(example, return_loss=False, estimate=True) -> (per-frame dicts, None)"""

    def __init__(self, dets, device):
        super().__init__()
        self.dets, self.device = dets, device

    def forward(self, example, return_loss=True, **kwargs):
        out = []
        for m in example["metadata"]:
            b, s, l = self.dets[m["index"]]
            out.append(dict(box3d_lidar=torch.from_numpy(b).to(self.device), scores=torch.from_numpy(s).to(self.device),
                            label_preds=torch.from_numpy(l).to(self.device), metadata=m))
        return out, None


class ShardLoader:
    def __init__(self, indices, batch):
        self.indices, self.batch = list(indices), batch
        self.sampler = self.indices
        self.dataset = self.indices

    def __iter__(self):
        for s in range(0, len(self.indices), self.batch):
            yield {"metadata": [{"index": i} for i in self.indices[s:s + self.batch]]}


def expected(dets, refs, device, same_class):
    """``box_iou_best`` on the whole pool in one call -> the dict ``sweep_iou_targets`` returns"""
    from al3d import selector_ops as ops
    from al3d.models.bbox_heads import pack_detections
    preds = PlantedDetector(dets, device)({"metadata": [{"index": i} for i in range(len(dets))]})[0]
    boxes, scores, labels, counts = pack_detections(preds)
    rb, rl, _, roff = refs.batch(range(len(dets)), device)
    iou, ref = ops.box_iou_best(boxes, labels, counts, rb, rl, roff, metric="iou3d", ref_rot_col=8, same_class=same_class)
    k = [len(d[1]) for d in dets]
    pick = lambda t: np.concatenate([t[i, 0, :k[i]].cpu().numpy() for i in range(len(dets))])      # noqa: E731
    return dict(off=np.concatenate([[0], np.cumsum(k)]), best_iou=pick(iou), best_ref=pick(ref), scores=pick(scores),
                labels=pick(labels))


def same(got, want):
    return all(np.array_equal(np.asarray(got[k]), np.asarray(want[k]).astype(np.asarray(got[k]).dtype)) for k in want)


def main():
    out_dir = sys.argv[1]
    dist.init_process_group(backend="gloo", init_method="env://")
    rank, world = dist.get_rank(), dist.get_world_size()
    from al3d.selectors.prepass import FrameRefs, sweep_iou_targets
    dev = torch.device("cuda", 0)
    dets, gt = planted_pool()
    refs = FrameRefs.from_frames(N_FRAMES, gt)
    per = (N_FRAMES + world - 1) // world
    mine = list(range(rank * per, min(N_FRAMES, (rank + 1) * per)))
    rec = {"rank": rank, "world": world, "rows": len(mine)}
    for same_class in (False, True):
        got = sweep_iou_targets(PlantedDetector(dets, dev), ShardLoader(mine, 2), dev, refs, same_class=same_class)
        want = expected(dets, refs, dev, same_class)
        rec[f"ok_{int(same_class)}"] = bool(same(got, want))
        rec[f"matched_{int(same_class)}"] = int((got["best_ref"] >= 0).sum())
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(rec, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
