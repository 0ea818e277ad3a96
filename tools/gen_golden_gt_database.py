#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Golden vectors for the ground-truth database builder -> tests/golden/gt_database.npz.

Runs the reference's own ``create_groundtruth_database`` (det3d/datasets/utils/create_gt_database.py:19-160), unmodified,
on a synthetic on-disk pool of 3 frames (key file + 2 of 3 listed sweeps each, <= ~2,000 merged points; 70 boxes in frame
0 so the kernels' 64-box tile is crossed, 0 boxes in frame 1, 14 in frame 2 of which two hold no point), twice: with the
defaults, and with ``used_classes`` + ``relative_path=False``.  Needs the reference tree (build container only).

Stand-ins, none with algorithmic content (oracle/ref_import.py has the rest: no numba, so the ``njit`` functions run as the
python they are, on numpy float32 scalars -- every product and sum of the sign rule is rounded to float32):

* ``det3d.datasets.dataset_factory.get_dataset`` returns a stand-in dataset (the real ones import the devkit).  Its
  ``get_sensor_data`` builds the ``res`` dict of nuscenes.py:156-172 and runs the reference's ``LoadPointCloudFromFile``
  and ``LoadPointCloudAnnotations`` on it;
* ``np.random.choice`` is pinned to list order while the reference runs (its sweep order is a fresh draw per frame);
* ``surface_equ_3d_jitv2`` (geometry.py:380-405) reads ``surfaces[0, 0, 0]`` before its loops, which numba does not
  bounds-check; as plain python it raises IndexError for a frame with no box, so a frame of zero boxes gets the empty
  result its loops would leave.  Every frame that has a box goes through the function itself.

Stored: arrays and strings only.  The raw files and infos of the pool, the merged points, the boxes, the reference's planes
(``surface_equ_3d_jitv2`` output), the ``points_in_rbbox`` masks, every ``.bin``'s contents, both dbinfos flattened in dict
order, and an edge block run through ``points_in_rbbox`` alone: an axis-aligned box with exactly representable faces and
points exactly on a face, an edge and a corner (outside: ``sign >= 0``), a point inside two overlapping boxes, a zero-size
box, a NaN point and a NaN box.

Margin.  For the random part every (point, box) pair must be decided with room: in float64, an inside pair has
``sign_k < -1e-4 |n_k|`` on all six planes, an outside pair ``sign_k > 1e-4 |n_k|`` on at least one.  Raw points whose
merged image fails are redrawn (the share is printed; more than 1 % stops the script).  The edge block is exempt: it is
exact by construction."""
import importlib
import os
import pickle
import shutil
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import as R  # noqa: E402
from gen_golden_sweeps import import_loading, rigid  # noqa: E402

NSWEEPS, SUFFIX = 3, "g"
CLASSES = ["car", "pedestrian", "truck", "traffic_cone"]
USED = ["pedestrian", "car"]


def import_reference():
    loading = import_loading()
    bno = sys.modules["det3d.core"].box_np_ops
    geometry = importlib.import_module("det3d.core.bbox.geometry")
    inner = geometry.surface_equ_3d_jitv2

    def surface_equ_3d_jitv2(surfaces):
        if surfaces.shape[0] == 0:
            return (np.zeros((0, surfaces.shape[1], 3), dtype=surfaces.dtype),
                    np.zeros((0, surfaces.shape[1]), dtype=surfaces.dtype))
        return inner(surfaces)

    geometry.surface_equ_3d_jitv2 = surface_equ_3d_jitv2

    class StandInDataset:
        def __init__(self, info_path, root_path, pipeline, test_mode, nsweeps=0):
            with open(info_path, "rb") as f:
                self._nusc_infos = pickle.load(f)
            self._root_path, self.test_mode, self.nsweeps = root_path, test_mode, nsweeps
            self.pipeline = [getattr(loading, c["type"])(**{k: v for k, v in c.items() if k != "type"}) for c in pipeline]

        def __len__(self):
            return len(self._nusc_infos)

        def get_sensor_data(self, idx):
            info = self._nusc_infos[idx]
            res = {"lidar": {"type": "lidar", "points": None, "nsweeps": self.nsweeps, "annotations": None},
                   "metadata": {"image_prefix": self._root_path, "num_point_features": 5, "token": info["token"]},
                   "calib": None, "cam": {}, "mode": "val" if self.test_mode else "train"}
            for t in self.pipeline:
                res, info = t(res, info)
            return res

    R._mod("det3d.datasets.dataset_factory", get_dataset=lambda name: StandInDataset)
    R._pkg("det3d.datasets.utils", os.path.join(R.REFERENCE_ROOT, "det3d", "datasets", "utils"))
    cgd = importlib.import_module("det3d.datasets.utils.create_gt_database")
    return cgd, bno, geometry, StandInDataset


class pinned_choice:
    """np.random.choice -> list order, while the reference runs."""

    def __enter__(self):
        self._orig = np.random.choice
        np.random.choice = lambda n, k, replace=False: np.arange(n)[:k]

    def __exit__(self, *a):
        np.random.choice = self._orig


def draw_points(rng, n):
    p = np.empty((n, 5), dtype=np.float32)
    p[:, :2] = rng.uniform(-18, 18, (n, 2))
    p[:, 2] = rng.uniform(-2.0, 1.0, n)
    p[:, 3] = rng.integers(0, 256, n)
    p[:, 4] = rng.integers(0, 32, n)
    return p


def make_pool(rng, tmp):
    """3 frames x (key + 3 listed sweeps); -> raws {name: [n, 5]}, infos (absolute paths: the reference opens them as is)."""
    raws, infos = {}, []
    for f in range(3):
        names = [f"f{f}_s{s}.bin" for s in range(4)]
        for s, nm in enumerate(names):
            n = int(rng.integers(560, 680))
            raws[nm] = draw_points(rng, n)
            raws[nm][:8, :2] = rng.uniform(-0.99, 0.99, (8, 2))      # remove_close drops these from the sweeps, not the key
        sweeps = [dict(lidar_path=os.path.join(tmp, names[s]), transform_matrix=None if (f, s) == (2, 1) else small_rigid(rng),
                       time_lag=float(0.05 * s + rng.uniform(0, 0.01))) for s in range(1, 4)]
        infos.append(dict(lidar_path=os.path.join(tmp, names[0]), sweeps=sweeps, token=f"tok{f}"))
    return raws, infos


def small_rigid(rng):
    T = rigid(rng)
    yaw = rng.uniform(-0.05, 0.05)
    T[:3, :3] = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    T[:3, 3] = rng.uniform(-1, 1, 3) * [1, 1, 0.05]
    return T


def draw_boxes(rng, merged, n, n_empty):
    """float64 rows as in real infos (``.astype(float32)`` is the loader's): centred on merged points, so they hold some."""
    b = np.empty((n, 9))
    pick = rng.choice(len(merged), n, replace=False)
    b[:, :3] = merged[pick, :3] + rng.normal(0, 0.2, (n, 3))
    b[:, 3:6] = rng.uniform([0.4, 0.4, 0.8], [3.0, 6.0, 3.0], (n, 3))
    b[:, 6:8] = rng.normal(0, 2, (n, 2))
    b[:, 8] = rng.uniform(-np.pi, np.pi, n)
    b[:n_empty, :2] += 200.0                                          # objects without a point: an empty file each
    return b


def write_files(tmp, raws):
    for nm, a in raws.items():
        a.tofile(os.path.join(tmp, nm))


def margins(points, planes):
    """float64 signs / |n| -> per (point, box): decided with room?"""
    x = points[:, :3].astype(np.float64)
    n, d = planes[..., :3].astype(np.float64), planes[..., 3].astype(np.float64)
    s = np.einsum("pc,bkc->pbk", x, n) + d[None]
    s /= np.linalg.norm(n, axis=-1)[None]
    return (s < -1e-4).all(-1) | (s > 1e-4).any(-1)


def flatten(db, tmp):
    keys = ["name", "path", "image_idx", "gt_idx", "box3d_lidar", "num_points_in_gt", "difficulty", "group_id"]
    rows = [e for v in db.values() for e in v]
    assert all(list(e.keys()) == keys for e in rows)
    out = {"class_order": np.array(list(db.keys())), "keys": np.array(keys),
           "types": np.array([type(rows[0][k]).__name__ for k in keys]),
           "difficulty_dtype": np.array(str(np.asarray(rows[0]["difficulty"]).dtype)),
           "name": np.array([str(e["name"]) for e in rows]),
           "path": np.array([e["path"].replace(tmp, "{root}") for e in rows]),
           "box3d_lidar": np.stack([e["box3d_lidar"] for e in rows])}
    assert out["box3d_lidar"].dtype == np.float32
    for k in ("image_idx", "gt_idx", "num_points_in_gt", "difficulty", "group_id"):
        out[k] = np.array([int(e[k]) for e in rows], dtype=np.int64)
    return out


def edge_block():
    nan = np.nan
    boxes = np.array([
        [1.0, 2.0, 0.5, 2.0, 4.0, 1.0, 0, 0, 0.0],           # faces x = 0, 2; y = 0, 4; z = 0, 1: exact
        [1.5, 2.0, 0.5, 2.0, 2.0, 2.0, 0, 0, 0.0],           # overlaps box 0 in x [0.5, 2], y [1, 3], z [0, 1]
        [1.0, 1.0, 0.5, 0.0, 0.0, 0.0, 0, 0, 0.3],           # zero size: holds nothing
        [1.0, 2.0, 0.5, 2.0, nan, 1.0, 0, 0, 0.0],           # NaN size
        [nan, 2.0, 0.5, 2.0, 4.0, 1.0, 0, 0, 0.0],           # NaN centre: every sign NaN -> holds every point
        [8.0, 8.0, 0.0, 1.0, 1.0, 1.0, 0, 0, 0.7],           # far away, rotated
    ], dtype=np.float32)
    pts = np.array([
        [1.0, 1.0, 0.5], [1.0, 2.0, 0.5],                    # inside box 0 only / inside boxes 0 and 1
        [0.0, 1.0, 0.5], [2.0, 1.0, 0.5], [1.0, 0.0, 0.5], [1.0, 4.0, 0.5], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0],   # on the faces
        [0.0, 0.0, 0.5], [2.0, 4.0, 1.0], [0.0, 0.0, 0.0],   # on an edge, on corners
        [1.0, 1.0, 0.5], [1.0, 1.0, 0.5],                    # the zero-size box's centre, twice
        [nan, 1.0, 0.5], [1.0, nan, 0.5], [1.0, 1.0, nan],   # NaN points
        [8.0, 8.0, 0.0], [3.0, 3.0, 3.0], [-1.0, 2.0, 0.5],
        [np.nextafter(np.float32(0), np.float32(1)), 1.0, 0.5], [np.nextafter(np.float32(2), np.float32(0)), 1.0, 0.5],
    ], dtype=np.float32)
    pts = np.concatenate([pts, np.arange(len(pts), dtype=np.float32)[:, None], np.zeros((len(pts), 1), np.float32)], 1)
    return pts, boxes


def main():
    cgd, bno, geometry, StandIn = import_reference()
    rng = np.random.default_rng(20261021)
    tmp = tempfile.mkdtemp(prefix="al3d_gtdb_")
    try:
        raws, infos = make_pool(rng, tmp)
        write_files(tmp, raws)
        for info in infos:                                   # annotations come after the first merge (boxes sit on points)
            info.update(gt_boxes=np.zeros((0, 9)), gt_names=np.array([], dtype="<U32"), gt_boxes_token=np.array([], dtype="<U32"),
                        gt_boxes_velocity=np.zeros((0, 3)))
        info_path = os.path.join(tmp, f"infos_train_{NSWEEPS:02d}sweeps_withvelo_{SUFFIX}.pkl")

        def merged_frames():
            with open(info_path, "wb") as f:
                pickle.dump(infos, f)
            ds = StandIn(info_path, tmp, [{"type": "LoadPointCloudFromFile", "dataset": "NuScenesDataset"},
                                          {"type": "LoadPointCloudAnnotations", "with_bbox": True}], True, NSWEEPS)
            with pinned_choice():
                return [ds.get_sensor_data(i) for i in range(len(ds))]

        first = merged_frames()
        for f, (nb, ne) in enumerate([(70, 1), (0, 0), (14, 2)]):
            b = draw_boxes(rng, first[f]["lidar"]["combined"], nb, ne)
            infos[f].update(gt_boxes=b, gt_names=np.array(rng.choice(CLASSES, nb), dtype="<U32"),
                            gt_boxes_token=np.array([f"b{f}_{i}" for i in range(nb)], dtype="<U32"),
                            gt_boxes_velocity=b[:, 6:8].copy())
        infos[2]["gt_names"][:3] = ["truck", "car", "truck"]

        def planes_of(boxes):
            corners = bno.center_to_corner_box3d(boxes[:, :3], boxes[:, 3:6], boxes[:, -1])
            n, d = geometry.surface_equ_3d_jitv2(bno.corner_to_surfaces_3d(corners)[:, :, :3, :])
            return np.concatenate([n, d[..., None]], axis=-1)

        # ---- margin: redraw the raw points whose merged image is decided too closely
        total = sum(len(a) for a in raws.values())
        redrawn = 0
        for _ in range(20):
            frames = merged_frames()
            bad_rows = []
            for f, res in enumerate(frames):
                boxes = res["lidar"]["annotations"]["boxes"]
                if len(boxes) == 0:
                    continue
                ok = margins(res["lidar"]["combined"], planes_of(boxes)).all(1)
                # merged row -> (file, raw row): the key file whole, then the first NSWEEPS - 1 sweeps without the close points
                where = []
                for s in range(NSWEEPS):
                    nm = f"f{f}_s{s}.bin"
                    a = raws[nm]
                    keep = np.ones(len(a), bool) if s == 0 else ~((np.abs(a[:, 0]) < 1.0) & (np.abs(a[:, 1]) < 1.0))
                    where += [(nm, r) for r in np.flatnonzero(keep)]
                assert len(where) == len(ok)
                bad_rows += [where[i] for i in np.flatnonzero(~ok)]
            if not bad_rows:
                break
            redrawn += len(bad_rows)
            for nm, r in bad_rows:
                raws[nm][r] = draw_points(rng, 1)[0]
            write_files(tmp, raws)
        else:
            raise SystemExit("margin: still failing after 20 rounds")
        print(f"margin: redrew {redrawn} of {total} raw points ({100.0 * redrawn / total:.3f} %)")
        assert redrawn <= 0.01 * total, "more than 1 % of the points had to be redrawn"

        # ---- the reference, unmodified, twice
        with pinned_choice():
            cgd.create_groundtruth_database("NUSC", tmp, info_path, nsweeps=NSWEEPS, suffix=SUFFIX)
        db_dir = os.path.join(tmp, f"gt_database_{NSWEEPS}sweeps_withvelo_{SUFFIX}")
        with open(os.path.join(tmp, f"dbinfos_train_{NSWEEPS}sweeps_withvelo_{SUFFIX}.pkl"), "rb") as f:
            db = pickle.load(f)
        file_names = sorted(os.listdir(db_dir))
        files = [np.fromfile(os.path.join(db_dir, n), dtype=np.float32).reshape(-1, 5) for n in file_names]
        alt_dir, alt_pkl = os.path.join(tmp, "alt_db"), os.path.join(tmp, "alt.pkl")
        with pinned_choice():
            cgd.create_groundtruth_database("NUSC", tmp, info_path, used_classes=USED, db_path=Path(alt_dir),
                                            dbinfo_path=alt_pkl, relative_path=False, nsweeps=NSWEEPS, suffix=SUFFIX)
        with open(alt_pkl, "rb") as f:
            db_alt = pickle.load(f)
        assert sorted(os.listdir(alt_dir)) == file_names

        out = {"nsweeps": np.int64(NSWEEPS), "suffix": np.array(SUFFIX), "used_classes": np.array(USED),
               "raw_names": np.array(list(raws.keys())),
               "raw_off": np.cumsum([0] + [len(a) for a in raws.values()]).astype(np.int64),
               "raw_data": np.concatenate(list(raws.values())),
               "file_names": np.array(file_names), "file_off": np.cumsum([0] + [len(a) for a in files]).astype(np.int64),
               "file_data": np.concatenate(files)}
        for k, v in flatten(db, tmp).items():
            out[f"db_{k}"] = v
        for k, v in flatten(db_alt, tmp).items():
            out[f"alt_{k}"] = v
        with pinned_choice():
            frames = merged_frames()
        for f, (res, info) in enumerate(zip(frames, infos)):
            pts, boxes = res["lidar"]["combined"], res["lidar"]["annotations"]["boxes"]
            assert pts.dtype == np.float32 and boxes.dtype == np.float32
            out[f"f{f}_points"], out[f"f{f}_boxes"] = pts, boxes
            out[f"f{f}_gt_boxes"] = info["gt_boxes"]                               # the float64 rows of the infos
            out[f"f{f}_gt_names"] = info["gt_names"]
            out[f"f{f}_planes"] = planes_of(boxes)
            out[f"f{f}_mask"] = bno.points_in_rbbox(pts, boxes)
            out[f"f{f}_lidar"] = np.array(os.path.basename(info["lidar_path"]))
            out[f"f{f}_sweep_files"] = np.array([os.path.basename(s["lidar_path"]) for s in info["sweeps"]])
            out[f"f{f}_time_lag"] = np.array([s["time_lag"] for s in info["sweeps"]])
            out[f"f{f}_has_xform"] = np.array([s["transform_matrix"] is not None for s in info["sweeps"]], dtype=np.uint8)
            out[f"f{f}_xform"] = np.stack([np.eye(4) if s["transform_matrix"] is None else s["transform_matrix"]
                                           for s in info["sweeps"]])
            print(f"frame {f}: {len(pts)} points, {len(boxes)} boxes, members {out[f'f{f}_mask'].sum(0).tolist()}")
        ep, eb = edge_block()
        with np.errstate(invalid="ignore"):
            out["edge_points"], out["edge_boxes"], out["edge_planes"] = ep, eb, planes_of(eb)
            out["edge_mask"] = bno.points_in_rbbox(ep, eb)
        print("edge mask:\n", out["edge_mask"].astype(int))
        path = os.path.join(ROOT, "tests", "golden", "gt_database.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
