"""Streaming sweep loader: real (or synthetic on-disk) nuScenes frames straight from their ``.bin`` files.

The reference overlaps 8 DataLoader worker processes with the GPU (det3d/datasets/loader/build_loader.py:23-59):
each worker reads the key frame + 9 sweeps of a sample, filters / transforms / concatenates them with numpy
(det3d/datasets/pipelines/loading.py:17-63,98-126) and pickles the result to the trainer.  Here

* a native reader pool (csrc/reader.cpp, ``al3d_reader_*``) preads the files of a whole BATCH into one pinned
  staging buffer, ``depth`` batches ahead of the GPU,
* one asynchronous H2D copy per batch moves the raw bytes,
* ``al3d_merge_sweeps_batch_f32`` does remove_close / float64 transform / time column / compaction for all frames of
  the batch at once (bit-identical per frame to the single-frame kernel and to the reference loader's golden),
* the device voxelizer turns the merged clouds into the ``example`` dict the detector reads,

so under the sweep's two-stream pipeline (``al3d/sweep.py``) file I/O, upload, merge and voxelization of batch i+1 all
run while batch i is convolved.  ``FileSweepLoader`` is a drop-in for ``DeviceSweepLoader`` (same example keys).
"""
import ctypes
import os

import numpy as np
import torch

from .. import lib
from ..detector_ops import build_voxelizer


def _cfg_get(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def usable_cores():
    """Cores this process may really use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period))))
    except Exception:
        pass
    return n


class SweepFileReader:
    """ctypes face of the native reader pool."""

    def __init__(self, threads=8):
        self._h = ctypes.c_void_p()
        lib.call("al3d_reader_create", int(threads), ctypes.byref(self._h))

    def close(self):
        if self._h:
            lib.load().al3d_reader_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _paths(paths):
        return (ctypes.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])

    def plan(self, paths):
        """-> int64 rows per file (whole 20-byte records; the reference drops a trailing partial row)."""
        rows = np.zeros(len(paths), dtype=np.int64)
        total = lib.load().al3d_reader_plan(self._paths(paths), len(paths), rows.ctypes.data_as(ctypes.c_void_p))
        if total < 0:
            lib.check(int(total), "al3d_reader_plan")
        return rows

    def submit(self, paths, row_off, rows, dst_ptr, dst_bytes):
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        job = lib.load().al3d_reader_submit(self._h, self._paths(paths), len(paths),
                                            row_off.ctypes.data_as(ctypes.c_void_p),
                                            rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dst_ptr),
                                            int(dst_bytes))
        if job < 0:
            lib.check(int(job), "al3d_reader_submit")
        return int(job)

    def wait(self, job):
        lib.call("al3d_reader_wait", self._h, int(job))


class _Staged:
    """One batch in flight on the host side: its pinned buffer, layout and read job."""
    __slots__ = ("pinned", "job", "total", "nf", "B", "o_off", "o_xf", "o_tl", "o_has", "o_key", "o_ff", "nbytes",
                 "ids", "slot", "extra")                     # extra: a subclass's own per-batch state (camera decode jobs)


class FileSweepLoader:
    """Batches of ``example`` dicts (voxelnet.py:84-97 keys) read from the frames' ``.bin`` files.

    ``infos``: nuScenes info dicts (``lidar_path``, ``sweeps[i]{lidar_path, transform_matrix, time_lag}``,
    nusc_common.py:410-419).  Sweep order = list order (the reference draws a fresh random order per sample and is
    therefore not reproducible)."""

    def __init__(self, infos, voxel_cfg, anchors, batch_size=8, device="cuda", nsweeps=10, root=None, threads=8,
                 indices=None, depth=2, min_distance=1.0, with_points=False, view=None, with_targets=False, target_cfg=None,
                 train_cfg=None):
        self.with_points = bool(with_points)   # also yield the padded point slots (``voxels``) for PillarFeatureNet
        # also yield the training targets of every batch (``labels`` / ``reg_targets`` / ``reg_weights`` / ``gt_index`` per
        # task, [B, A_t]...) from the infos' ``gt_boxes`` / ``gt_names``: one al3d_assign_targets_f32 launch per batch.
        # ``target_cfg``: the config's ``assigner`` dict (box_coder, target_assigner, out_size_factor), as AssignTarget takes
        self.with_targets = bool(with_targets)
        if self.with_targets and target_cfg is None:
            raise ValueError("with_targets=True needs target_cfg (the config's assigner dict)")
        self._target_cfg = target_cfg
        self._target_plan = None
        # ``train_cfg``: the config's ``train_preprocessor`` dict.  Every batch then goes through ONE
        # datasets.augment.augment_batch between the sweep merge and the voxelizer (GT-AUG sampling, per-object noise, flips,
        # global rotation / scale, shuffle), the boxes through Voxelization's range filter, and the targets are assigned from
        # the boxes that are left; ``gt_boxes`` / ``gt_names`` / ``gt_classes`` per frame join the example.  The sampler's
        # ``.bin`` paths are relative to ``root``.  Costs one more host read per batch (the merged frames' sizes).
        self._train_aug = None
        if train_cfg is not None:
            if not self.with_targets:
                raise ValueError("train_cfg needs with_targets=True")
            from .augment import TrainAugmenter
            self._train_aug = TrainAugmenter(train_cfg)
            self._bv_range = np.array(_cfg_get(voxel_cfg, "range"), dtype=np.float32)[[0, 1, 3, 4]]
        # (flip_x, flip_y, rot, scale): the merged points of every batch are augmented in place before they are voxelized
        # (selector_ops.points_view_, CALD's second sweep); None launches nothing
        self.view = view
        self.infos = infos
        self.batch_size = int(batch_size)
        self.device = torch.device(device)
        self.nsweeps, self.root, self.min_distance = int(nsweeps), root, float(min_distance)
        self.indices = list(range(len(infos))) if indices is None else list(indices)
        self.depth = max(1, int(depth))
        # hard voxelizer, or the dynamic one when the config's caps are -1 (refuses with_points before any thread starts)
        self.voxelizer = build_voxelizer(voxel_cfg, self.batch_size, self.device, with_points=self.with_points)
        self.reader = SweepFileReader(threads)
        self.anchors = [torch.as_tensor(a, dtype=torch.float32, device=self.device) for a in (anchors or [])]
        self.dataset = infos
        self.sampler = self.indices
        # ring of depth + 1 pinned buffers: the one being uploaded is never the one being refilled
        self._pinned = [None] * (self.depth + 1)
        self._upload_done = [None] * (self.depth + 1)
        self.bytes_read = 0

    def __len__(self):
        return (len(self.indices) + self.batch_size - 1) // self.batch_size

    def _path(self, p):
        p = str(p)
        return p if self.root is None or os.path.isabs(p) else os.path.join(self.root, p)

    # transform rule of al3d_merge_sweeps_batch_rule_f32: 0 = det3d's loader (one float64 4 x 4 product, rounded once)
    rule = 0

    def _frame_files(self, info):
        """One frame's files in merge order: (paths, 3x4 / 4x4 float64 transforms or None, time lags, key-frame flags).
        det3d infos (nusc_common.py:410-419): ``lidar_path``, ``sweeps[i]{lidar_path, transform_matrix, time_lag}``."""
        assert self.nsweeps - 1 <= len(info["sweeps"]), \
            f"nsweeps {self.nsweeps} should not greater than list length {len(info['sweeps'])}."
        paths, xforms, lags, keys = [self._path(info["lidar_path"])], [None], [0.0], [1]
        for k in range(self.nsweeps - 1):
            sw = info["sweeps"][k]
            paths.append(self._path(sw["lidar_path"]))
            xforms.append(sw.get("transform_matrix"))
            lags.append(float(sw["time_lag"]))
            keys.append(0)
        return paths, xforms, lags, keys

    def _start(self, b):
        """Plan batch b, lay out its staging buffer, start the reads (returns immediately)."""
        ids = self.indices[b * self.batch_size:(b + 1) * self.batch_size]
        paths, xforms, lags, keys, first = [], [], [], [], [0]
        for i in ids:
            p_, x_, l_, k_ = self._frame_files(self.infos[i])
            paths += p_
            xforms += x_
            lags += l_
            keys += k_
            first.append(len(paths))
        rows = self.reader.plan(paths)
        st = _Staged()
        st.ids, st.nf, st.B = ids, len(paths), len(ids)
        st.total = int(rows.sum())
        o = st.total * 20
        o += (-o) % 8
        st.o_off = o
        o += 8 * (st.nf + 1)
        st.o_xf = o
        o += 96 * st.nf
        st.o_tl = o
        o += 8 * st.nf
        st.o_has = o
        o += st.nf
        st.o_key = o
        o += st.nf
        o += (-o) % 4
        st.o_ff = o
        o += 4 * (st.B + 1)
        st.nbytes = o
        st.slot = b % len(self._pinned)
        if self._upload_done[st.slot] is not None:       # the buffer's previous upload must have left the host
            self._upload_done[st.slot].synchronize()
            self._upload_done[st.slot] = None
        if self._pinned[st.slot] is None or self._pinned[st.slot].numel() < st.nbytes:
            self._pinned[st.slot] = torch.empty(int(st.nbytes * 1.25) + 4096, dtype=torch.uint8).pin_memory()
        st.pinned = self._pinned[st.slot]
        host = st.pinned.numpy()
        off = host[st.o_off:st.o_xf].view(np.int64)
        off[0] = 0
        np.cumsum(rows, out=off[1:])
        xf = host[st.o_xf:st.o_tl].view(np.float64).reshape(st.nf, 12)
        has = host[st.o_has:st.o_has + st.nf]
        for i, t in enumerate(xforms):
            has[i] = 0 if t is None else 1
            xf[i] = 0.0 if t is None else np.asarray(t, dtype=np.float64)[:3, :].reshape(12)
        host[st.o_tl:st.o_has].view(np.float64)[:] = lags
        host[st.o_key:st.o_key + st.nf] = keys
        host[st.o_ff:st.o_ff + 4 * (st.B + 1)].view(np.int32)[:] = first
        st.job = self.reader.submit(paths, off[:-1], rows, st.pinned.data_ptr(), st.total * 20)
        self.bytes_read += st.total * 20
        return st

    def _finish(self, st):
        """Wait for the reads of a staged batch, upload, merge, voxelize -> example dict."""
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
        rg = getattr(self, "point_range", None)              # PointsRangeFilter of the BEVFusion test pipeline (else None)
        rg = None if rg is None else (ctypes.c_float * 6)(*[float(np.float32(v)) for v in rg])
        lib.call("al3d_merge_sweeps_batch_range_f32", base, base + st.o_off, st.nf, st.total, base + st.o_xf, base + st.o_has,
                 base + st.o_tl, base + st.o_key, base + st.o_ff, st.B, self.min_distance, int(self.rule), rg, out.data_ptr(),
                 frame_off.data_ptr(), ws.data_ptr(), stream.cuda_stream)
        if self.view is not None:
            from ..selector_ops import points_view_
            points_view_(out[:st.total], self.view)
        gt = None
        if self._train_aug is not None:
            out, frame_off, gt = self._augment(st.ids, out, frame_off)
        v = self.voxelizer(out, frame_off, want_voxels=self.with_points)
        gs = self.voxelizer.grid_size
        ex = {
            "voxel_features": v["feat"], "coordinates": v["coords"], "num_points": v["num_points"],
            "num_voxels": v["num_voxels"], "voxel_cap": v["voxel_cap"],
            "shape": np.tile(np.asarray(gs, dtype=np.int64)[None], (st.B, 1)),
            "anchors": self.anchors,
            "metadata": [{"token": str(self.infos[i].get("token", f"frame{i:06d}")), "index": i} for i in st.ids],
            "points": out, "point_offsets": frame_off,
        }
        if self.with_points:
            ex["voxels"] = v["voxels"]
        if self.with_targets:
            ex.update(self._targets(st.ids, gt))
            if gt is not None:
                ex.update(gt_boxes=[g["gt_boxes"] for g in gt], gt_names=[g["gt_names"] for g in gt],
                          gt_classes=[g["gt_classes"] for g in gt])
        if "point2voxel" in v:              # dynamic voxelizer: each point's row, what DynamicPillarFeatureNet pools by
            ex["point2voxel"] = v["point2voxel"]
        return ex

    def _augment(self, ids, points, frame_off):
        """The train Preprocess of the batch's frames and Voxelization's range filter on their boxes (preprocess.py:57-256,
        282-288) -> (points, frame offsets, per-frame annotations)."""
        from .augment import augment_batch, filter_gt_box_outside_range
        offs = frame_off.cpu().tolist()
        frames = [dict(points=points[offs[b]:offs[b + 1]], boxes=np.asarray(self.infos[i]["gt_boxes"]).astype(np.float32),
                       names=self.infos[i]["gt_names"], image_prefix=self.root, num_point_features=5, flip_both=True)
                  for b, i in enumerate(ids)]
        gt = augment_batch(frames, self._train_aug)
        for g in gt:
            g.pop("points")
            mask = filter_gt_box_outside_range(g["gt_boxes"], self._bv_range)
            for k in g:
                g[k] = g[k][mask]
        off = torch.from_numpy(self._train_aug.batch_offsets).to(self.device)
        return self._train_aug.batch_points, off, gt

    def _targets(self, ids, gt=None):
        """AssignTarget's train branch for the batch's frames (preprocess.py:380-479) from their infos.  A box whose name is
        in no task keeps its row and matches nothing (the reference's Preprocess removes it beforehand, ``gt_boxes_mask``);
        ``gt_index`` counts the info's own rows."""
        from ..detector_ops import assign_targets
        if self._target_plan is None:
            from .target_assigner import build_assign_plan
            gs = np.asarray(self.voxelizer.grid_size)
            fm = [*(gs[:2] // _cfg_get(self._target_cfg, "out_size_factor")), 1][::-1]
            self._target_plan, _ = build_assign_plan(self._target_cfg, fm, self.device)
        nd = self._target_plan.n_dim
        boxes, names = [], []
        for b, i in enumerate(ids):
            g = np.asarray(self.infos[i]["gt_boxes"] if gt is None else gt[b]["gt_boxes"], dtype=np.float32).reshape(-1, 9)
            boxes.append(np.ascontiguousarray(g if nd == 9 else g[:, [0, 1, 2, 3, 4, 5, 8]]))
            names.append(self.infos[i]["gt_names"] if gt is None else gt[b]["gt_names"])
        out = assign_targets(self._target_plan, boxes, gt_names=names)
        return {k: out[k] for k in ("labels", "reg_targets", "reg_weights", "gt_index")}

    def __iter__(self):
        nb = len(self)
        staged = {}
        try:
            for b in range(min(self.depth, nb)):
                staged[b] = self._start(b)
            for b in range(nb):
                st = staged.pop(b)
                ex = self._finish(st)
                if b + self.depth < nb:
                    staged[b + self.depth] = self._start(b + self.depth)   # read ahead while batch b runs downstream
                yield ex
        finally:
            # abandoned midway (exception downstream, break, a second iter()): the reads already submitted still
            # write into pinned slots the next iteration will reuse -- wait them out before anyone can
            for st in staged.values():
                try:
                    self.reader.wait(st.job)
                except Exception:
                    pass
                self._abandon(st)
            staged.clear()

    def _abandon(self, st):
        """Hook: a staged batch that will never be finished (subclasses drop what they attached to it)."""
