#!/usr/bin/env python3
"""Measure the ground-truth database builder on an on-disk pool of tools/write_synthetic_pool.py:

    python tools/bench_gt_database.py --root /dev/shm/al3d_gtdb_pool --scenes 2 --boxes 40 --batch-size 4

Prints one JSON line:

* ``numpy``: the same frames through the numpy yardstick (the host loader of al3d/datasets/nusc_files.py, the float32 sign
  rule, the per-object gather and the file writes) on the host cores, one process per core, frames/s -- run FIRST, before
  this process touches the GPU (the workers are forked);
* ``database``: ``create_groundtruth_database`` from the files to the database and its pickle, frames/s (wall clock,
  the median of ``--repeats`` runs and all of them);
* ``count_ms`` / ``gather_ms``: the two launches per batch, from device events around each (median over the batches of
  one pass, after a warm-up pass), next to the points and boxes per batch.

The frames' boxes are drawn here (the synthetic pool's are all zero): ``--boxes`` per frame, traffic-sized, centred on
points of the frame so that they hold some."""
import argparse
import json
import multiprocessing
import os
import pickle
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def draw_boxes(infos, root, n_boxes, nsweeps, seed=0):
    from al3d.datasets.nusc_files import load_frame_points
    rng = np.random.default_rng(seed)
    cache = {}
    for info in infos:
        key = info["lidar_path"]
        if key not in cache:
            cache[key] = load_frame_points(info, nsweeps=nsweeps, root=root)[:, :3]
        pts = cache[key]
        b = np.zeros((n_boxes, 9))
        b[:, :3] = pts[rng.choice(len(pts), n_boxes)] + rng.normal(0, 0.3, (n_boxes, 3))
        b[:, 3:6] = rng.uniform([0.5, 0.5, 1.0], [2.5, 6.0, 3.0], (n_boxes, 3))
        b[:, 8] = rng.uniform(-np.pi, np.pi, n_boxes)
        info["gt_boxes"] = b
        info["gt_names"] = np.array(rng.choice(["car", "truck", "pedestrian"], n_boxes), dtype="<U32")


def _numpy_frame(job):
    """One frame the reference's way, vectorised: load, test, gather, write."""
    from al3d.datasets.nusc_files import load_frame_points
    from al3d.detector_ops import box_planes
    index, info, root, nsweeps, out_dir = job
    points = load_frame_points(info, nsweeps=nsweeps, root=root)
    boxes = info["gt_boxes"].astype(np.float32)
    planes = box_planes(boxes)
    x, y, z = points[:, None, 0], points[:, None, 1], points[:, None, 2]
    inside = np.ones((len(points), len(boxes)), dtype=bool)
    for k in range(6):
        n = planes[None, :, k]
        inside &= ~((((x * n[..., 0] + y * n[..., 1]) + z * n[..., 2]) + n[..., 3]) >= 0)
    total = 0
    for i in range(len(boxes)):
        g = points[inside[:, i]]
        g[:, :3] -= boxes[i, :3]
        g[:, :5].tofile(os.path.join(out_dir, f"{index}_{info['gt_names'][i]}_{i}.bin"))
        total += len(g)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default="/dev/shm/al3d_gtdb_pool")
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--base", type=int, default=8)
    ap.add_argument("--boxes", type=int, default=40)
    ap.add_argument("--nsweeps", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--numpy-frames", type=int, default=32, help="frames of the pool the numpy leg runs (0: skip it)")
    ap.add_argument("--procs", type=int, default=0, help="numpy worker processes (0: the usable cores, at most 16)")
    a = ap.parse_args()

    from write_synthetic_pool import write_pool
    from al3d.datasets.file_loader import usable_cores
    infos, _ = write_pool(a.root, a.scenes, base=a.base, nsweeps=a.nsweeps)
    draw_boxes(infos, a.root, a.boxes, a.nsweeps)
    info_path = os.path.join(a.root, f"infos_train_{a.nsweeps:02d}sweeps_withvelo_bench.pkl")
    with open(info_path, "wb") as f:
        pickle.dump(infos, f)
    out = {"frames": len(infos), "boxes_per_frame": a.boxes, "nsweeps": a.nsweeps, "batch_size": a.batch_size}

    # ---- the numpy yardstick on the host cores (forked workers: before the GPU is opened here)
    if a.numpy_frames > 0:
        procs = a.procs or min(usable_cores(), 16)
        nf = min(a.numpy_frames, len(infos))
        np_dir = os.path.join(a.root, "numpy_db")
        os.makedirs(np_dir, exist_ok=True)
        jobs = [(i, infos[i], a.root, a.nsweeps, np_dir) for i in range(nf)]
        with multiprocessing.get_context("fork").Pool(procs) as pool:
            pool.map(_numpy_frame, jobs[:procs])                  # warm the page cache and the workers
            t0 = time.perf_counter()
            members = pool.map(_numpy_frame, jobs, chunksize=1)
            dt = time.perf_counter() - t0
        out["numpy"] = {"frames": nf, "procs": procs, "frames_per_s": round(nf / dt, 2), "members": int(sum(members))}
        shutil.rmtree(np_dir, ignore_errors=True)

    # ---- files -> database
    import torch
    from al3d import selector_ops as ops
    from al3d.datasets import SweepPointsLoader, create_groundtruth_database
    from al3d.detector_ops import box_planes
    runs = []
    for r in range(a.repeats + 1):                                # the first run warms up and is dropped
        db_dir = os.path.join(a.root, f"bench_db_{r}")
        t0 = time.perf_counter()
        db = create_groundtruth_database("NUSC", a.root, info_path, db_path=db_dir, dbinfo_path=os.path.join(a.root, f"bench_{r}.pkl"),
                                         nsweeps=a.nsweeps, suffix="bench", lidar_root=a.root, batch_size=a.batch_size)
        runs.append(time.perf_counter() - t0)
        members = sum(e["num_points_in_gt"] for v in db.values() for e in v)
        shutil.rmtree(db_dir, ignore_errors=True)
    runs = runs[1:]
    out["database"] = {"frames_per_s": round(len(infos) / float(np.median(runs)), 2),
                       "all_frames_per_s": [round(len(infos) / t, 2) for t in runs],
                       "members": int(members)}
    if "numpy" in out and out["numpy"]["frames"] == len(infos):
        out["same_member_count_as_numpy"] = out["numpy"]["members"] == out["database"]["members"]

    # ---- the two launches, device events
    dev = torch.device("cuda")
    count_ms, gather_ms, pts_n, box_n = [], [], [], []
    for rep in range(2):
        loader = SweepPointsLoader(infos, batch_size=a.batch_size, device=dev, nsweeps=a.nsweeps, root=a.root)
        for points, point_off, ids in loader:
            boxes = np.concatenate([infos[i]["gt_boxes"].astype(np.float32) for i in ids])
            box_off = torch.from_numpy(np.cumsum([0] + [len(infos[i]["gt_boxes"]) for i in ids]).astype(np.int32)).to(dev)
            planes = torch.from_numpy(box_planes(boxes)).to(dev)
            centres = torch.from_numpy(np.ascontiguousarray(boxes[:, :3])).to(dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            counts, ws, _ = ops.points_in_boxes_count(points, point_off, planes, box_off)
            ev[1].record()
            offsets = torch.zeros(len(boxes) + 1, dtype=torch.int64, device=dev)
            torch.cumsum(counts, 0, out=offsets[1:])
            total = int(offsets[-1])
            ev[2].record()
            ops.points_in_boxes_gather(points, point_off, planes, box_off, offsets, centres, ws, total, 5)
            ev[3].record()
            torch.cuda.synchronize()
            if rep == 1:
                count_ms.append(ev[0].elapsed_time(ev[1]))
                gather_ms.append(ev[2].elapsed_time(ev[3]))
                pts_n.append(int(point_off[-1]))
                box_n.append(len(boxes))
        loader.reader.close()
    out["count_ms"] = {"median": round(float(np.median(count_ms)), 4), "min": round(min(count_ms), 4), "max": round(max(count_ms), 4)}
    out["gather_ms"] = {"median": round(float(np.median(gather_ms)), 4), "min": round(min(gather_ms), 4), "max": round(max(gather_ms), 4)}
    out["batches"] = len(count_ms)
    out["points_per_batch"] = int(np.median(pts_n))
    out["boxes_per_batch"] = int(np.median(box_n))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
