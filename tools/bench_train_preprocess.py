#!/usr/bin/env python3
"""Measure the train Preprocess at the workload's shape: a 10-sweep cloud (~250k points), ~40 annotated and ~15 sampled boxes:

    python tools/bench_train_preprocess.py --batch 4 --repeats 20

Prints one JSON line:

* ``frames_per_s``: ``datasets.augment.augment_batch`` end to end (host sampling and draws, uploads, the three launches, the
  host read) for batches of ``--batch`` frames, wall clock with a synchronise at the end, median of ``--repeats``;
* ``noise_ms`` / ``count_ms`` / ``points_ms``: ``al3d_noise_per_box_f32``, ``al3d_augment_points_count_f32`` and
  ``al3d_augment_points_f32`` alone on one batch's arrays, device events around each call (median / min / max);
* ``host_ms``: the rest of the call (frames_per_s's time per batch minus the three kernels).

The database is synthetic and written under ``--root``: 60 objects per class with 20 to 400 points each."""
import argparse
import json
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CLASSES = ["car", "truck", "bus", "pedestrian", "barrier"]
SIZES = dict(car=[1.97, 4.63, 1.74], truck=[2.51, 6.93, 2.84], bus=[2.94, 10.5, 3.47], pedestrian=[0.67, 0.73, 1.77],
             barrier=[2.53, 0.5, 0.98])


def draw_boxes(rng, n):
    names = rng.choice(CLASSES, n)
    b = np.zeros((n, 9), np.float32)
    b[:, :2], b[:, 2] = rng.uniform(-50, 50, (n, 2)), rng.uniform(-2, 0, n)
    b[:, 3:6] = np.array([SIZES[k] for k in names]) * rng.uniform(0.85, 1.2, (n, 3))
    b[:, 6:8], b[:, 8] = rng.normal(0, 2, (n, 2)), rng.uniform(-np.pi, np.pi, n)
    return b, np.array(names, dtype="<U32")


def write_database(root, rng, per_class=60):
    os.makedirs(os.path.join(root, "db"), exist_ok=True)
    db = {}
    for name in CLASSES:
        boxes, _ = draw_boxes(rng, per_class)
        boxes[:, 3:6] = np.array(SIZES[name]) * rng.uniform(0.85, 1.2, (per_class, 3))
        db[name] = []
        for i, b in enumerate(boxes):
            n = int(rng.integers(20, 400))
            pts = np.zeros((n, 5), np.float32)
            pts[:, :3] = rng.uniform(-0.45, 0.45, (n, 3)) * b[3:6]
            rel = f"db/{name}_{i}.bin"
            pts.tofile(os.path.join(root, rel))
            db[name].append(dict(name=name, path=rel, image_idx=0, gt_idx=i, box3d_lidar=b, num_points_in_gt=n,
                                 difficulty=np.int32(0), group_id=i))
    path = os.path.join(root, "dbinfos.pkl")
    with open(path, "wb") as f:
        pickle.dump(db, f)
    return path


def timed(fn, repeats, torch):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--points", type=int, default=250000)
    ap.add_argument("--boxes", type=int, default=40)
    ap.add_argument("--root", default="/dev/shm/al3d_train_prep_bench")
    a = ap.parse_args()

    import torch
    from al3d.datasets import augment as A
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    pkl = write_database(a.root, rng)
    cfg = dict(mode="train", shuffle_points=True, gt_loc_noise=[0.0, 0.0, 0.0], gt_rot_noise=[0.0, 0.0],
               global_rot_noise=[-0.3925, 0.3925], global_scale_noise=[0.95, 1.05], global_rot_per_obj_range=[0, 0],
               remove_points_after_sample=True, remove_unknown_examples=False, remove_environment=False, class_names=CLASSES,
               db_sampler=dict(type="GT-AUG", db_info_path=pkl, sample_groups=[{c: a.boxes // len(CLASSES) + 3} for c in CLASSES],
                               db_prep_steps=[dict(filter_by_min_num_points={c: 5 for c in CLASSES}), dict(filter_by_difficulty=[-1])],
                               global_random_rotation_range_per_object=[0, 0], rate=1.0))
    np.random.seed(0)
    aug = A.TrainAugmenter(cfg)
    frames = []
    for _ in range(a.batch):
        pts = np.zeros((a.points, 5), np.float32)
        pts[:, :2], pts[:, 2] = rng.normal(0, 20, (a.points, 2)), rng.uniform(-3, 1, a.points)
        b, names = draw_boxes(rng, a.boxes)
        frames.append(dict(points=torch.from_numpy(pts).to(dev), boxes=b, names=names, image_prefix=a.root,
                           num_point_features=5, flip_both=True))
    A.augment_batch(frames, aug, keep_debug=True)
    torch.cuda.synchronize()
    d = aug.last
    sampled_boxes = [int(d["box_off"][i + 1] - d["box_off"][i]) - a.boxes for i in range(a.batch)]
    walls = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        A.augment_batch(frames, aug)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    wall = sorted(walls)[len(walls) // 2]

    # the three entries alone, on arrays of the batch's shape
    R, T, P = int(d["box_off"][-1]), aug.num_try, int(d["point_off"][-1])
    pts = d["input"]
    b = np.concatenate([draw_boxes(rng, int(d["box_off"][i + 1] - d["box_off"][i]))[0] for i in range(a.batch)])
    rot, loc = np.zeros((R, T)), np.zeros((R, T, 3))
    h = A._noise_inputs(b, np.ones(R, bool), loc, rot)
    t = {k: A._up(v, v.dtype, dev) for k, v in h.items()}
    t["cos"], t["sin"], t["loc"] = t["cos"].reshape(R, T), t["sin"].reshape(R, T), t["loc"].reshape(R, T, 3)
    box_off = A._up(d["box_off"], np.int32, dev)
    point_off = A._up(d["point_off"], np.int64, dev)
    sampled_off = A._up(np.array(d["sampled"]), np.int64, dev)
    noise = timed(lambda: A.noise_per_box_device(t["corners"], t["centres2"], t["valid"], t["cos"], t["sin"], t["loc"], box_off), a.repeats, torch)
    count = timed(lambda: A.augment_points_count(pts, point_off, sampled_off, t["planes"], box_off), a.repeats, torch)
    drop, kept, ws, _ = A.augment_points_count(pts, point_off, sampled_off, t["planes"], box_off)
    n_out = kept.cpu().numpy().astype(np.int64)
    out_off = A._up(np.cumsum(np.concatenate([[0], n_out])), np.int64, dev)
    total = int(n_out.sum())
    rows = A._up(np.concatenate([rng.permutation(int(n)) for n in n_out]), np.int32, dev)
    sel, _ = A.noise_per_box_device(t["corners"], t["centres2"], t["valid"], t["cos"], t["sin"], t["loc"], box_off)
    xf = torch.tensor([[0.98, 0.2, 1.01]] * a.batch, dtype=torch.float32, device=dev)
    flip = torch.ones((a.batch, 2), dtype=torch.uint8, device=dev)
    points = timed(lambda: A.augment_points(pts, point_off, out_off, total, xf, drop_mask=drop, workspace=ws, planes=t["planes"],
                                            box_off=box_off, valid=t["valid"], centres=t["centres3"], rot_cos=t["cos"],
                                            rot_sin=t["sin"], loc=t["loc"], selected=sel, flip=flip, rows=rows), a.repeats, torch)
    kernels = noise["median"] + count["median"] + points["median"]
    print(json.dumps(dict(batch=a.batch, points_per_frame=P // a.batch, boxes_per_frame=a.boxes, sampled_boxes=sampled_boxes,
                          num_try=T, frames_per_s=a.batch / wall, batch_ms=wall * 1e3, noise_ms=noise, count_ms=count,
                          points_ms=points, host_ms=wall * 1e3 - kernels, device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
