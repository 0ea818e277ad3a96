"""The ground-truth database of one active-learning round (reference det3d/datasets/utils/create_gt_database.py:19-160,
``tools/create_data.py nuscenes_data_prep --suffix S``): every annotated object's points, box-relative, one ``.bin`` per
object, and the ``dbinfos`` pickle the training sampler reads.

The reference walks the frames one at a time on the host: ``LoadPointCloudFromFile`` (ten ``np.fromfile`` + a float64
transform each), then ``points_in_rbbox`` and a boolean gather per object.  Here the frames stream through the native
reader pool and the batched sweep merge (``SweepPointsLoader``: ``FileSweepLoader`` without a voxelizer), a batch's
(point, box) tests and the per-box compaction are two launches (``selector_ops.points_in_boxes``,
csrc/points_in_boxes.hip) with one host read between them, and the files are written by a small thread pool while the
next batch runs.  The pickle is written last and atomically, so an interrupted run never looks complete.

Sweep order is list order, as everywhere here: the reference draws ``np.random.choice`` per frame."""
import os
import pickle
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from .. import lib
from .file_loader import FileSweepLoader, SweepFileReader

POINT_FEATURES = 5          # NUSC (create_gt_database.py:76-77)


class SweepPointsLoader(FileSweepLoader):
    """``FileSweepLoader``'s reading, upload and merge, and nothing after: yields ``(points [P, 5] f32, point_off [B+1]
    i64, ids)`` on the device per batch of frames."""

    def __init__(self, infos, batch_size=4, device="cuda", nsweeps=10, root=None, threads=8, indices=None, depth=2,
                 min_distance=1.0):
        self.infos = infos
        self.batch_size = int(batch_size)
        self.device = torch.device(device)
        self.nsweeps, self.root, self.min_distance = int(nsweeps), root, float(min_distance)
        self.indices = list(range(len(infos))) if indices is None else list(indices)
        self.depth = max(1, int(depth))
        self.reader = SweepFileReader(threads)
        self._pinned = [None] * (self.depth + 1)
        self._upload_done = [None] * (self.depth + 1)
        self.bytes_read = 0

    def _finish(self, st):
        self.reader.wait(st.job)
        dev = self.device
        stream = torch.cuda.current_stream(dev)
        buf = torch.empty(max(st.nbytes, 1), dtype=torch.uint8, device=dev)
        buf[:st.nbytes].copy_(st.pinned[:st.nbytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
        self._upload_done[st.slot] = ev
        out = torch.empty((max(st.total, 1), 5), dtype=torch.float32, device=dev)
        frame_off = torch.empty((st.B + 1,), dtype=torch.int64, device=dev)
        ws = torch.empty(lib.load().al3d_merge_sweeps_workspace_bytes(st.total), dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        lib.call("al3d_merge_sweeps_batch_f32", base, base + st.o_off, st.nf, st.total, base + st.o_xf, base + st.o_has,
                 base + st.o_tl, base + st.o_key, base + st.o_ff, st.B, self.min_distance, out.data_ptr(),
                 frame_off.data_ptr(), ws.data_ptr(), stream.cuda_stream)
        return out, frame_off, st.ids


def database_paths(data_path, nsweeps, suffix=None, db_path=None, dbinfo_path=None):
    """The NUSC names of create_gt_database.py:58-69 -> ``(db_path, dbinfo_path)`` as ``Path``."""
    root = Path(data_path)
    tail = f"{nsweeps}sweeps_withvelo" if suffix is None else f"{nsweeps}sweeps_withvelo_{suffix}"
    db_path = root / f"gt_database_{tail}" if db_path is None else Path(db_path)
    dbinfo_path = root / f"dbinfos_train_{tail}.pkl" if dbinfo_path is None else Path(dbinfo_path)
    return db_path, dbinfo_path


def _write_bin(path, rows):
    with open(path, "wb") as f:
        f.write(rows.tobytes())


class GtDatabaseWriter:
    """The host half (create_gt_database.py:101-160): file names, ``db_info`` dicts in the reference's key order and
    types, the group counter that advances only for kept objects, files on a thread pool, the pickle last."""

    def __init__(self, db_path, dbinfo_path, relative_path=True, used_classes=None, writers=4):
        self.db_path, self.dbinfo_path = Path(db_path), Path(dbinfo_path)
        self.relative_path, self.used_classes = relative_path, used_classes
        self.db_path.mkdir(parents=True, exist_ok=True)
        if self.dbinfo_path.exists():           # a pickle of an earlier run must not vouch for this run's files
            self.dbinfo_path.unlink()
        self.all_db_infos = {}
        self.group_counter = 0
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(writers)))
        self._pending = []

    def add_frame(self, image_idx, names, gt_boxes, rows):
        """One frame: ``names [n]``, ``gt_boxes [n, 9]`` f32, ``rows``: per object its ``[k, 5]`` f32 points (box-relative,
        ascending point index).  Starts the file writes and returns."""
        group_dict = {}
        group_ids = np.arange(gt_boxes.shape[0], dtype=np.int64)
        difficulty = np.zeros(gt_boxes.shape[0], dtype=np.int32)
        for i in range(gt_boxes.shape[0]):
            filename = f"{image_idx}_{names[i]}_{i}.bin"
            filepath = self.db_path / filename
            gt_points = rows[i]
            self._pending.append(self._pool.submit(_write_bin, filepath, gt_points))
            if (self.used_classes is None) or names[i] in self.used_classes:
                db_info = {
                    "name": names[i],
                    "path": str(self.db_path.stem + "/" + filename) if self.relative_path else str(filepath),
                    "image_idx": image_idx,
                    "gt_idx": i,
                    "box3d_lidar": gt_boxes[i],
                    "num_points_in_gt": int(gt_points.shape[0]),
                    "difficulty": difficulty[i],
                }
                local_group_id = group_ids[i]
                if local_group_id not in group_dict:
                    group_dict[local_group_id] = self.group_counter
                    self.group_counter += 1
                db_info["group_id"] = group_dict[local_group_id]
                self.all_db_infos.setdefault(names[i], []).append(db_info)

    def drain(self, keep=0):
        """Wait for all but the newest ``keep`` file writes; a failed write raises here."""
        while len(self._pending) > keep:
            self._pending.pop(0).result()

    def close(self):
        """All files down, then the pickle: to a temporary name, then renamed."""
        try:
            self.drain()
        finally:
            self._pool.shutdown(wait=True)
        tmp = self.dbinfo_path.with_name(self.dbinfo_path.name + ".tmp")
        with open(tmp, "wb") as f:
            pickle.dump(self.all_db_infos, f)
        os.replace(tmp, self.dbinfo_path)

    def abort(self):
        for fut in self._pending:
            fut.cancel()
        self._pool.shutdown(wait=True)


def _load_infos(info_path):
    with open(info_path, "rb") as f:
        infos = pickle.load(f)
    if isinstance(infos, dict):                  # nuscenes.py:98-104 (test_mode)
        infos = [i for v in infos.values() for i in v]
    return infos


def create_groundtruth_database(
    dataset_class_name,
    data_path,
    info_path=None,
    used_classes=None,
    db_path=None,
    dbinfo_path=None,
    relative_path=True,
    add_rgb=False,
    lidar_only=False,
    bev_only=False,
    coors_range=None,
    **kwargs,
):
    """Same signature and defaults as the reference.  ``kwargs``: ``nsweeps`` (1 without it, as there), ``suffix``; ours:
    ``batch_size`` (4 frames a batch), ``device``, ``threads`` (file readers), ``writers`` (file writers), ``lidar_root``
    (joined in front of relative ``lidar_path`` entries; the reference opens them as they are).  Returns the dbinfos."""
    if dataset_class_name != "NUSC":
        raise NotImplementedError(f"create_groundtruth_database: dataset {dataset_class_name!r} is not built -- only "
                                  "\"NUSC\" (the KITTI / Lyft branches are out of scope)")
    if add_rgb:
        raise NotImplementedError("create_groundtruth_database: add_rgb is not built (the reference never reads it either)")
    if bev_only:
        raise NotImplementedError("create_groundtruth_database: bev_only is not built (the reference never reads it either)")
    from .. import selector_ops as ops
    nsweeps = int(kwargs["nsweeps"]) if "nsweeps" in kwargs else 1
    assert nsweeps > 0, "At least input one sweep please!"
    db_path, dbinfo_path = database_paths(data_path, nsweeps, kwargs.get("suffix", None), db_path, dbinfo_path)
    infos = _load_infos(info_path)
    device = torch.device(kwargs.get("device", "cuda"))
    loader = SweepPointsLoader(infos, batch_size=kwargs.get("batch_size", 4), device=device, nsweeps=nsweeps,
                               root=kwargs.get("lidar_root", None), threads=kwargs.get("threads", 8))
    writer = GtDatabaseWriter(db_path, dbinfo_path, relative_path, used_classes, kwargs.get("writers", 4))
    batches = iter(loader)
    try:
        for points, point_off, ids in batches:
            boxes = [np.asarray(infos[i]["gt_boxes"]).astype(np.float32).reshape(-1, 9) for i in ids]
            names = [infos[i]["gt_names"] for i in ids]
            box_off = np.zeros(len(ids) + 1, dtype=np.int32)
            np.cumsum([len(b) for b in boxes], out=box_off[1:])
            all_boxes = np.concatenate(boxes, axis=0) if boxes else np.zeros((0, 9), np.float32)
            # count, one host read of the total, gather: rows of box r are rows[off[r]:off[r + 1]], ascending point index
            rows, _, _, offsets = ops.points_in_boxes(points, point_off, all_boxes, torch.from_numpy(box_off).to(device),
                                                      POINT_FEATURES)
            rows, off = rows.cpu().numpy(), offsets.cpu().numpy()
            writer.drain(keep=0)                 # the previous batch's files (written while this one was read and tested)
            for k, index in enumerate(ids):
                r0, r1 = int(box_off[k]), int(box_off[k + 1])
                writer.add_frame(index, names[k], boxes[k], [rows[off[r]:off[r + 1]] for r in range(r0, r1)])
        writer.close()
    except BaseException:
        writer.abort()
        raise
    finally:
        batches.close()                          # waits out the reads already submitted (FileSweepLoader.__iter__)
        loader.reader.close()
    print("dataset length: ", len(infos))
    for k, v in writer.all_db_infos.items():
        print(f"load {len(v)} {k} database infos")
    return writer.all_db_infos
