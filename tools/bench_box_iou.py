#!/usr/bin/env python3
"""Times the box IoU / NMS ops (csrc/box_iou.hip) on the device and prints one JSON line per measurement.

    python tools/bench_box_iou.py [--repeats 5] [--out profiles/box_iou.jsonl]

1. the IoU matrix at 4,096 x 4,096 (frame-like boxes: most pairs are disjoint), early reject on and off, alternated;
2. the best-IoU entry at the sweep's shape (128 frames x 6 tasks x 83 slots against ~40 reference rows per frame), against
   the only alternative there is without it: a per-frame loop over the matrix entry plus ``torch.max``;
3. the NMS at 1,000 and 4,096 candidates;
4. a dense matrix (every pair overlaps: 4,096 boxes in one 30 m cluster) -- what the clip costs when nothing is rejected.

Every figure is device time between two events around ``calls`` back-to-back calls, after a warm-up of the same shape, the
median of ``--repeats`` windows with their spread; pairs/s = pairs the call decides over that time.  Inputs are seeded."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

FOOT = np.array([(0.41, 0.41), (0.67, 0.73), (0.60, 1.70), (0.77, 2.11), (2.53, 0.50), (1.97, 4.63), (2.51, 6.93), (2.94, 10.5)])


def boxes(rng, n, extent, dim=7):
    b = np.zeros((n, dim), np.float32)
    b[:, :2] = rng.uniform(-extent, extent, (n, 2))
    b[:, 2] = rng.uniform(-1.5, 0.0, n)
    b[:, 3:5] = FOOT[rng.integers(0, len(FOOT), n)] * rng.uniform(0.8, 1.2, (n, 1))
    b[:, 5] = rng.uniform(1.0, 2.5, n)
    b[:, dim - 1] = rng.uniform(-np.pi, np.pi, n)
    return b


def timed(fn, calls, repeats):
    """-> (median ms per call, min, max) over ``repeats`` windows of ``calls`` calls"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from al3d import selector_ops as ops
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    lines = []

    def report(name, ms, pairs, **extra):
        rec = dict(name=name, ms=round(ms[0], 4), ms_min=round(ms[1], 4), ms_max=round(ms[2], 4), pairs=int(pairs),
                   pairs_per_s=float(f"{pairs / (ms[0] * 1e-3):.4g}"), **extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    # 1 + 4: the matrix
    for name, extent in (("matrix_4096x4096_frame", 54.0), ("matrix_4096x4096_dense", 15.0)):
        a, b = (torch.from_numpy(boxes(rng, 4096, extent)).to(dev) for _ in range(2))
        share = float((ops.box_iou_matrix(a, b, metric="overlap_bev") > 0).float().mean())
        on = ops.box_iou_matrix(a, b, metric="iou3d")
        off = ops.box_iou_matrix(a, b, metric="iou3d", launch=(16, 256, 0))
        same = bool(torch.equal(on.view(torch.int32), off.view(torch.int32)))
        for _ in range(2):                                   # alternated: other work shares the machine
            for tag, launch in (("reject_on", (16, 256, 1)), ("reject_off", (16, 256, 0))):
                ms = timed(lambda: ops.box_iou_matrix(a, b, metric="iou3d", launch=launch), 20, args.repeats)
                report(f"{name}_{tag}", ms, 4096 * 4096, overlapping_share=round(share, 5), same_bits=same)
    # 2: the sweep's shape
    B, nt, post, nref = 128, 6, 83, 40
    pred = torch.from_numpy(boxes(rng, B * nt * post, 54.0, dim=9).reshape(B, nt, post, 9)).to(dev)
    labels = torch.from_numpy(rng.integers(0, 10, (B, nt, post)).astype(np.int32)).to(dev)
    counts = torch.from_numpy(rng.integers(20, post + 1, (B, nt)).astype(np.int32)).to(dev)
    per = rng.integers(nref - 15, nref + 16, B)
    off_h = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
    ref = torch.from_numpy(boxes(rng, int(off_h[-1]), 54.0)).to(dev)
    ref_labels = torch.from_numpy(rng.integers(0, 10, int(off_h[-1])).astype(np.int32)).to(dev)
    ref_off = torch.from_numpy(off_h).to(dev)
    pairs = int((counts.cpu().numpy().sum(1) * per).sum())

    def best():
        return ops.box_iou_best(pred, labels, counts, ref, ref_labels, ref_off, metric="iou3d")

    def loop():
        out = []
        for b in range(B):
            m = ops.box_iou_matrix(pred[b].reshape(nt * post, 9), ref[off_h[b]:off_h[b + 1]], metric="iou3d", rot_col=8, rot_col_b=6)
            out.append(m.max(1))
        return out
    v, r = best()
    lv = torch.stack([x.values for x in loop()]).reshape(B, nt, post)
    valid = torch.arange(post, device=dev)[None, None] < counts[:, :, None]
    same = bool(torch.equal(v[valid].view(torch.int32), lv[valid].view(torch.int32)))
    for _ in range(2):
        report("best_iou_128x6x83_vs_40", timed(best, 20, args.repeats), pairs, same_values_as_loop=same)
        report("matrix_loop_plus_torch_max_128_frames", timed(loop, 2, args.repeats), pairs)
    # 3: the NMS (clusters of up to four boxes, as a head's candidates come)
    for n in (1000, 4096):
        centres = rng.uniform(-54, 54, (n // 3 + 1, 2)).repeat(3, axis=0)[:n]
        b = boxes(rng, n, 0.0)
        b[:, :2] = centres + rng.uniform(-1.0, 1.0, (n, 2))
        bt, st = torch.from_numpy(b).to(dev), torch.from_numpy(rng.uniform(0, 1, n).astype(np.float32)).to(dev)
        kept = int(ops.nms_boxes(bt, st, 0.2).numel())
        report(f"nms_{n}", timed(lambda: ops.nms_boxes(bt, st, 0.2), 10, args.repeats), n * (n - 1) // 2, kept=kept)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
