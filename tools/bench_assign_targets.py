#!/usr/bin/env python3
"""Measure anchor target assignment at the CBGS shape (6 tasks / 10 classes, 128 x 128 x 2 anchors per class):

    python tools/bench_assign_targets.py --batch 128 --repeats 20

Prints one JSON line:

* ``kernel_ms``: ``al3d_assign_targets_f32`` alone for one batch, device events around the call (median / min / max of
  ``--repeats`` after a warm-up), the batch's boxes already on the device;
* ``call_ms``: ``detector_ops.assign_targets`` for the same batch, wall clock with a synchronise at the end: the host's near
  boxes, one upload, the launch;
* ``numpy_ms``: the vectorised numpy restatement (tests/assign_targets_numpy.py) of the same batch on one host core, measured
  on ``--numpy-frames`` frames and scaled to the batch;
* ``loader``: frames/s of ``FileSweepLoader`` over an on-disk synthetic pool with ``with_targets`` off and on (``--loader-
  frames`` > 0), the cost of the option.

The boxes: the synthetic pool's counts per frame (``synthetic.make_pool``: U{0..69}), classes drawn uniformly from the ten,
sizes around the class's anchor, centres inside the range."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def draw_frames(infos, gens, seed=0):
    rng = np.random.default_rng(seed)
    names, sizes = [g["class_name"] for g in gens], np.array([g["sizes"] for g in gens])
    frames = []
    for info in infos:
        n = len(info["gt_names"])
        k = rng.integers(len(names), size=n)
        b = np.zeros((n, 9), np.float32)
        b[:, :2] = rng.uniform(-50, 50, (n, 2))
        b[:, 2] = rng.uniform(-2, 0, n)
        b[:, 3:6] = sizes[k] * rng.uniform(0.85, 1.2, (n, 3))
        b[:, 6:8] = rng.normal(0, 2, (n, 2))
        b[:, 8] = rng.uniform(-np.pi, np.pi, n)
        frames.append((b, np.array([names[i] for i in k], dtype="<U32")))
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--numpy-frames", type=int, default=8, help="frames the numpy leg runs (0: skip it)")
    ap.add_argument("--loader-frames", type=int, default=0, help="frames of an on-disk pool for the loader leg (0: skip it)")
    ap.add_argument("--loader-batch", type=int, default=8)
    ap.add_argument("--root", default="/dev/shm/al3d_assign_pool")
    a = ap.parse_args()

    import torch
    import assign_targets_numpy as Y
    from al3d import synthetic
    from al3d.datasets.target_assigner import build_assign_plan
    from al3d.datasets.anchors import build_anchor_generator
    from al3d.detector_ops import assign_targets
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "cbgs_spatial_temporal_feature.py"))
    gens = cfg.target_assigner.anchor_generators
    infos, _ = synthetic.make_pool((a.batch + 39) // 40, seed=1)
    frames = draw_frames(infos[:a.batch], gens)
    dev = torch.device("cuda")
    plan, _ = build_assign_plan(cfg.assigner, (1, 128, 128), dev)
    boxes, names = [f[0] for f in frames], [f[1] for f in frames]
    out = {"batch": a.batch, "boxes": int(sum(len(b) for b in boxes)), "classes": len(plan.rows),
           "anchors": int(plan.anchors.shape[0]), "overlaps_per_batch": None}
    out["overlaps_per_batch"] = int(sum(2 * plan.rows[plan.class_index[n]]["num_loc"] * plan.rows[plan.class_index[n]]["num_rot"]
                                        for ns in names for n in ns))

    for _ in range(3):
        assign_targets(plan, boxes, gt_names=names)
    torch.cuda.synchronize()
    call = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        assign_targets(plan, boxes, gt_names=names)
        torch.cuda.synchronize()
        call.append((time.perf_counter() - t0) * 1e3)
    out["call_ms"] = {"median": round(float(np.median(call)), 3), "min": round(min(call), 3), "max": round(max(call), 3)}

    # the launch alone: the same arguments, prepared once
    import ctypes
    from al3d import lib
    from al3d.ops.box_np_ops import limit_period, rbbox2d_to_near_bbox
    flat = np.concatenate(boxes)
    flat[:, -1] = limit_period(flat[:, -1], 0.5, np.pi * 2)
    flat = np.nan_to_num(flat)
    bv = torch.from_numpy(np.ascontiguousarray(rbbox2d_to_near_bbox(flat[:, [0, 1, 3, 4, -1]]), dtype=np.float32)).to(dev)
    cls = torch.from_numpy(np.array([plan.class_index[n] for ns in names for n in ns], dtype=np.int32)).to(dev)
    d_boxes = torch.from_numpy(flat).to(dev)
    gt_off = np.cumsum([0] + [len(b) for b in boxes]).astype(np.int32)
    tab, rows, _ = plan.table(a.batch)
    lab = torch.empty(rows, dtype=torch.int32, device=dev)
    wgt = torch.empty(rows, dtype=torch.float32, device=dev)
    idx = torch.empty(rows, dtype=torch.int32, device=dev)
    tgt = torch.empty((rows, plan.code_size), dtype=torch.float32, device=dev)
    ovl = torch.empty(max(len(flat), 1), dtype=torch.float32, device=dev)
    args = [plan.anchors.data_ptr(), plan.anchors_bv.data_ptr(), plan.anchors.shape[0], 9, tab, len(plan.rows), d_boxes.data_ptr(),
            bv.data_ptr(), cls.data_ptr(), len(flat), gt_off.ctypes.data_as(ctypes.c_void_p), a.batch, 1, 0, 0, lab.data_ptr(),
            tgt.data_ptr(), wgt.data_ptr(), idx.data_ptr(), rows, ovl.data_ptr(), torch.cuda.current_stream().cuda_stream]
    kern = []
    for r in range(a.repeats + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.call("al3d_assign_targets_f32", *args)
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            kern.append(e0.elapsed_time(e1))
    out["kernel_ms"] = {"median": round(float(np.median(kern)), 4), "min": round(min(kern), 4), "max": round(max(kern), 4)}
    out["output_mb"] = round(rows * (12 + 4 * plan.code_size) / 1e6, 1)

    if a.numpy_frames > 0:
        tasks = []
        by = {g["class_name"]: g for g in gens}
        for t in cfg.tasks:
            classes = []
            for n in t["class_names"]:
                an = build_anchor_generator(by[n]).generate([1, 128, 128])
                classes.append(dict(class_name=n, anchors=an.reshape([*an.shape[:3], -1, an.shape[-1]]),
                                    matched=by[n]["matched_threshold"], unmatched=by[n]["unmatched_threshold"]))
            tasks.append(classes)
        nf = min(a.numpy_frames, a.batch)
        t0 = time.perf_counter()
        want = Y.assign_batch(tasks, dict(n_dim=9, vec=True, linear=False, norm_velo=False), frames[:nf])
        dt = (time.perf_counter() - t0) * 1e3
        out["numpy_ms"] = {"frames": nf, "per_frame": round(dt / nf, 2), "per_batch": round(dt / nf * a.batch, 1)}
        got = assign_targets(plan, boxes[:nf], gt_names=names[:nf])
        out["same_labels_as_numpy"] = all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got["labels"], want["labels"]))

    if a.loader_frames > 0:
        from write_synthetic_pool import write_pool
        from al3d.datasets import FileSweepLoader, generate_task_anchors
        linfos, _ = write_pool(a.root, (a.loader_frames + 39) // 40, base=8, nsweeps=10)
        linfos = linfos[:a.loader_frames]
        for info, (b, n) in zip(linfos, draw_frames(linfos, gens, seed=2)):
            info["gt_boxes"], info["gt_names"] = b, n
        anchors = generate_task_anchors(cfg.tasks, gens, [1, 128, 128])
        res = {}
        for key, kw in (("off", {}), ("on", dict(with_targets=True, target_cfg=cfg.assigner))):
            runs = []
            for r in range(3):
                loader = FileSweepLoader(linfos, cfg.voxel_generator, anchors, batch_size=a.loader_batch, device=dev, root=a.root, **kw)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for ex in loader:
                    pass
                torch.cuda.synchronize()
                runs.append(len(linfos) / (time.perf_counter() - t0))
                loader.reader.close()
            res[key] = {"frames_per_s": round(float(np.median(runs[1:])), 1), "all": [round(v, 1) for v in runs]}
        out["loader"] = dict(res, frames=len(linfos), batch_size=a.loader_batch)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
