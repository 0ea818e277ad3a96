"""The PPAL and CALD pre-passes: the files ``PPALSelector`` (``class_weight_file``) and ``CaldSelector`` (``buffer_path``,
``jsdiv_path``) replay, computed here instead of by the reference's separate tools.

Reference: ``tools/ppal_pred_list.py`` + ``tools/ppal_unc.py`` and ``tools/cald_pred_list.py`` + ``tools/cald_ent.py``.
Each pair sweeps the detector over the pool, matches every frame's detections to reference boxes with the nuScenes rule
(``classwise_weight/algo.py::accumulate``, ``classwise_weight_cald/algo.py``) and reduces the matches.  Here the matching
runs on the device beside the sweep, from the raw NMS buffers (``selector_ops.match_boxes``, csrc/box_match.hip); only the
``[N, ncls]`` per-class sums come back, and the closing formulas run on the host in float64.

* PPAL: reference boxes are the ground truth of ``infos_origin`` (``ref_scores`` = -1.0, the devkit's default for ground
  truth); ``ppal_class_weights`` turns the labelled frames' per-class match quality into class difficulty weights.
* CALD: a first sweep's detections are the reference boxes of a second sweep over an augmented view of the same clouds
  (``view = (flip_x, flip_y, rot, scale)``, applied by the loader, undone inside the matching kernel);
  ``cald_rankings`` turns the per-frame consistency and matched-class histogram into the two rankings.

Not built (as in ``selector_ops.match_boxes``): the bike-rack and ``num_pts == 0`` filters of the devkit's
``filter_eval_boxes`` -- they need devkit tables the infos files do not carry -- and the lidar -> global conversion, under
which centre distance and scale IoU are invariant.
"""
import json
import os
import pickle
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .base_selector import _rank

CALD_SLOTS = 10         # cald_ent.py:135,146 hard-codes ten class slots
# detection_cvpr_2019's class_range (the nuScenes devkit's published detection configuration), metres
NUSC_CLASS_RANGE = {"car": 50.0, "truck": 50.0, "bus": 50.0, "trailer": 50.0, "construction_vehicle": 50.0,
                    "pedestrian": 40.0, "motorcycle": 40.0, "bicycle": 40.0, "traffic_cone": 30.0, "barrier": 30.0}


def _rows(boxes, k, dim=9):
    """``boxes`` as ``[k, D]`` float32 (an empty frame has no width of its own)."""
    return np.asarray(boxes, np.float32).reshape(k, -1) if k else np.zeros((0, dim), np.float32)


class FrameRefs:
    """Reference boxes of a pool on the host, concatenated by frame in dataset order: ``boxes [R,>=6]`` f32 (columns 0, 1
    and 3, 4, 5 are read), ``labels [R]`` i32 (merged class id; -1 never matches), ``scores [R]`` f32, ``off [N+1]``."""

    def __init__(self, boxes, labels, scores, off):
        self.boxes = np.ascontiguousarray(boxes, dtype=np.float32)
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.scores = np.ascontiguousarray(scores, dtype=np.float32)
        self.off = np.ascontiguousarray(off, dtype=np.int64)
        assert self.boxes.ndim == 2 and self.boxes.shape[1] >= 6 and self.off[-1] == len(self.boxes) == len(self.labels)

    def __len__(self):
        return len(self.off) - 1

    @classmethod
    def from_frames(cls, num_frames, frames, dim=9):
        """``frames``: ``{dataset index: (boxes [K,D], labels [K], scores [K])}``; a frame that is absent has no boxes."""
        empty = (np.zeros((0, dim), np.float32), np.zeros((0,), np.int32), np.zeros((0,), np.float32))
        rows = [frames.get(i, empty) for i in range(num_frames)]
        rows = [(_rows(b, len(l), dim), l, s) for b, l, s in rows]
        dim = max([b.shape[1] for b, l, _ in rows if len(l)] or [dim])
        boxes = [np.pad(b, ((0, 0), (0, dim - b.shape[1]))) if len(l) else np.zeros((0, dim), np.float32)
                 for b, l, _ in rows] + [np.zeros((0, dim), np.float32)]
        off = np.concatenate([[0], np.cumsum([len(r[1]) for r in rows])])
        return cls(np.concatenate(boxes), np.concatenate([r[1] for r in rows] + [empty[1]]),
                   np.concatenate([r[2] for r in rows] + [empty[2]]), off)

    @classmethod
    def from_infos(cls, infos, class_names):
        """Ground truth of det3d infos (``gt_boxes [K,>=6]``, ``gt_names [K]``); a name outside ``class_names`` gets
        label -1.  Scores are -1.0, the devkit's default ``detection_score`` of a ground-truth box."""
        ids = {n: i for i, n in enumerate(class_names)}
        frames = {}
        for i, info in enumerate(infos):
            names = np.asarray(info["gt_names"])
            frames[i] = (_rows(info["gt_boxes"], len(names)), np.array([ids.get(str(n), -1) for n in names], np.int32),
                         np.full((len(names),), -1.0, np.float32))
        return cls.from_frames(len(infos), frames)

    def batch(self, ids, device):
        """The rows of frames ``ids`` as the four device tensors ``match_boxes`` takes."""
        rows = [np.arange(self.off[i], self.off[i + 1]) for i in ids]
        sel = np.concatenate(rows) if rows else np.zeros((0,), np.int64)
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        return (torch.from_numpy(self.boxes[sel]).to(device), torch.from_numpy(self.labels[sel]).to(device),
                torch.from_numpy(self.scores[sel]).to(device), torch.from_numpy(off).to(device))


def head_class_names(detector) -> List[str]:
    """The merged class list a head's ``label_preds`` index (task-major, like ``PPALSelector.buffer_pred``)."""
    names = detector.bbox_head.class_names
    return [c for group in names for c in group] if names and isinstance(names[0], (list, tuple)) else list(names)


def _raw_of(preds):
    """``(boxes, scores, labels, counts)`` of a batch's detections: the NMS buffers of a lazy list, or plain per-frame
    dicts packed to one task."""
    if hasattr(preds, "match"):
        boxes, scores, labels, counts, done, _ = preds._raw
        torch.cuda.current_stream(boxes.device).wait_event(done)
        return boxes, scores, labels, counts
    from ..models.bbox_heads import pack_detections
    return pack_detections(preds)


def _batches(detector, dataloader, device):
    """``(dataset indices, preds)`` per batch: the loop of ``PPALSelector.buffer_pred``."""
    from ..sweep import example_to_device
    sampler = list(getattr(dataloader, "sampler", []) or [])
    seen = 0
    with torch.no_grad():
        for batch in dataloader:
            example = example_to_device(batch, device)
            preds, _ = detector(example, return_loss=False, estimate=True)
            b = len(preds)
            yield (sampler[seen:seen + b] if sampler else list(range(seen, seen + b))), preds
            seen += b


def sweep_detections(detector, dataloader, device, num_frames) -> FrameRefs:
    """One sweep whose detections, read back once per batch, become reference boxes (CALD's first sweep).  Only the
    frames this rank's loader visits are filled: the second sweep visits the same ones."""
    frames = {}
    for ids, preds in _batches(detector, dataloader, device):
        boxes, scores, labels, counts = (t.cpu().numpy() for t in _raw_of(preds))
        for b, i in enumerate(ids):
            keep = [slice(0, min(max(int(c), 0), boxes.shape[2])) for c in counts[b]]
            frames[int(i)] = (np.concatenate([boxes[b, t, k] for t, k in enumerate(keep)]),
                              np.concatenate([labels[b, t, k] for t, k in enumerate(keep)]).astype(np.int32),
                              np.concatenate([scores[b, t, k] for t, k in enumerate(keep)]))
    return FrameRefs.from_frames(num_frames, frames)


def sweep_matches(detector, dataloader, device, refs: FrameRefs, view=None, ncls: Optional[int] = None,
                  class_range=None, origins=None, **kw) -> Dict[str, np.ndarray]:
    """One sweep that matches every frame's detections to ``refs`` and returns the per-frame arrays in dataset order:
    ``cls_count [N,ncls]`` i32, ``cls_quality`` / ``cls_cons [N,ncls]`` f32 (host).  ``view``: set on the loader for the
    sweep (it must take one: ``DeviceSweepLoader`` / ``FileSweepLoader``) and handed to the matching, which undoes it.
    ``class_range [ncls]`` + ``origins [N,2]`` (host, dataset order): the range rule; ``kw``: ``dist_th``, ``max_boxes``.
    Under ``torch.distributed`` every rank sweeps its loader's frames and the rows are all-gathered (a collective)."""
    from ..sweep import gather_in_dataset_order
    from .. import selector_ops as ops
    ncls = len(head_class_names(detector)) if ncls is None else int(ncls)
    n = len(refs)
    cr = None if class_range is None else torch.as_tensor(np.asarray(class_range, np.float32), device=device)
    if view is not None and not hasattr(dataloader, "view"):
        raise TypeError(f"{type(dataloader).__name__} takes no view")
    saved = getattr(dataloader, "view", None)
    if hasattr(dataloader, "view"):
        dataloader.view = view
    index, rows = [], {"cls_count": [], "cls_quality": [], "cls_cons": []}
    try:
        for ids, preds in _batches(detector, dataloader, device):
            args = dict(kw, ncls=ncls, view=view)
            if cr is not None:
                args.update(class_range=cr, origin=torch.as_tensor(
                    np.asarray(origins, np.float32)[list(ids)].reshape(len(ids), 2), device=device))
            r = refs.batch(ids, device)
            out = preds.match(r, **args) if hasattr(preds, "match") else ops.match_boxes(*_raw_of(preds), *r, **args)
            for k in rows:
                rows[k].append(out[k])
            index.extend(int(i) for i in ids)
    finally:
        if hasattr(dataloader, "view"):
            dataloader.view = saved
    idx = torch.as_tensor(index, dtype=torch.int64, device=device)
    res = {}
    for k, v in rows.items():
        local = torch.cat(v) if v else torch.empty((0, ncls), dtype=torch.int32 if k == "cls_count" else torch.float32,
                                                   device=device)
        res[k] = gather_in_dataset_order(local, idx, n).cpu().numpy()
    return res


def sweep_iou_targets(detector, dataloader, device, refs: FrameRefs, metric: str = "iou3d", same_class: bool = False,
                      convention: str = "det3d") -> Dict[str, np.ndarray]:
    """The Estimator's training targets (det3d/models/detectors/estimator.py:98-115: ``boxes_iou3d_gpu(pred, gt).max(1)``)
    for every detection of the pool: the loop of ``sweep_matches`` with ``selector_ops.box_iou_best`` on each batch's raw
    NMS buffers beside the sweep -- no IoU matrix is written.  ``refs``: the ground truth (``FrameRefs.from_infos``), angle
    in the last column like the detections'.  Returns, in dataset order, ``off [N+1]`` i64 and per detection ``best_iou``
    f32, ``best_ref`` i64 (row of ``refs.boxes``, -1 where the frame has no reference box -- of the detection's class under
    ``same_class``), ``scores`` f32 and ``labels`` i32 (host).  ``same_class=False`` is the reference's class-agnostic
    target.  Under ``torch.distributed`` every rank sweeps its loader's frames and the rows are all-gathered (a collective).

    Difference kept on purpose: the reference computes targets only for the boxes that contain a point
    (estimator.py:491); here every detection carries one, and a trainer drops the others."""
    import torch.distributed as dist
    from ..sweep import gather_in_dataset_order
    from .. import selector_ops as ops
    if refs.boxes.shape[1] < 7:
        raise ValueError(f"sweep_iou_targets: reference boxes need an angle column, got {refs.boxes.shape[1]} columns")
    n = len(refs)
    index, rows = [], {"best_iou": [], "best_ref": [], "scores": [], "labels": [], "valid": []}
    for ids, preds in _batches(detector, dataloader, device):
        boxes, scores, labels, counts = _raw_of(preds)
        rb, rl, _, roff = refs.batch(ids, device)
        iou, ref = ops.box_iou_best(boxes, labels, counts, rb, rl, roff, metric=metric, convention=convention,
                                    ref_rot_col=rb.shape[1] - 1, same_class=same_class)
        first = torch.as_tensor([int(refs.off[i]) for i in ids], dtype=torch.int64, device=device)
        ref = torch.where(ref >= 0, ref.long() - roff[:-1].long()[:, None, None] + first[:, None, None], ref.long())
        b, post = len(ids), boxes.shape[2]
        valid = (torch.arange(post, device=device)[None, None, :] < counts.clamp(0, post)[:, :, None]).reshape(b, -1)
        front = torch.argsort((~valid).to(torch.int8), dim=1, stable=True)      # a frame's detections first, order kept
        for k, v in (("best_iou", iou), ("best_ref", ref), ("scores", scores), ("labels", labels)):
            rows[k].append(v.reshape(b, -1).gather(1, front))
        rows["valid"].append(valid.sum(1, keepdim=True).to(torch.int32))
        index.extend(int(i) for i in ids)
    # batches (pack_detections) and ranks may differ in their slots per frame: one width for the gathers
    width = torch.tensor([max([r.shape[1] for r in rows["scores"]] or [0])], device=device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(width, op=dist.ReduceOp.MAX)        # a rank whose shard is empty still joins the gathers
    width = int(width)
    idx = torch.as_tensor(index, dtype=torch.int64, device=device)
    dtypes = dict(best_iou=torch.float32, best_ref=torch.int64, scores=torch.float32, labels=torch.int32, valid=torch.int32)
    full = {}
    for k, v in rows.items():
        w = 1 if k == "valid" else width
        v = [torch.nn.functional.pad(r.to(dtypes[k]), (0, w - r.shape[1])) for r in v]
        local = torch.cat(v) if v else torch.empty((0, w), dtype=dtypes[k], device=device)
        full[k] = gather_in_dataset_order(local, idx, n).cpu().numpy()
    keep = np.arange(width)[None, :] < full["valid"]
    res = {"off": np.concatenate([[0], np.cumsum(full["valid"][:, 0])]).astype(np.int64)}
    for k in ("best_iou", "best_ref", "scores", "labels"):
        res[k] = full[k][keep]
    return res


def run_iou_targets(detector, dataloader, device, infos, out_path, **kw):
    """``sweep_iou_targets`` against the ground truth of ``infos`` -> ``out_path`` (.npz, rank 0 writes)."""
    from .base_selector import master_only
    res = sweep_iou_targets(detector, dataloader, device, FrameRefs.from_infos(infos, head_class_names(detector)), **kw)

    @master_only
    def write():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        tmp = out_path + ".tmp.npz"
        np.savez(tmp, **res)
        os.replace(tmp, out_path)
    write()
    return res


# ------------------------------------------------------------------------------------------- closing formulas (host, f64)
def ppal_class_weights(cls_count, cls_quality, labelled: Sequence[int], class_names: Sequence[str], alpha: float = 3.0,
                       ub: float = 2.0) -> Dict[str, float]:
    """Class difficulty weights (ppal_unc.py:79-98): over the labelled frames' matches, ``mean_q`` = mean of
    ``score^0.6 * iou^0.4`` per class and the weight is ``1 + alpha * log(b * (1 - mean_q) + 1) * ub`` with
    ``b = exp(1 / alpha) - 1``.  A class with no match among the labelled frames is absent, as in the reference."""
    labelled = list(labelled)
    cnt = np.asarray(cls_count)[labelled].astype(np.int64).sum(axis=0)
    qual = np.asarray(cls_quality)[labelled].astype(np.float64).sum(axis=0)
    b = np.exp(1.0 / alpha) - 1
    out = {}
    for c, name in enumerate(class_names):
        if cnt[c] > 0:
            reverse_q = 1.0 - qual[c] / cnt[c]
            out[str(name)] = float(1 + alpha * np.log(b * reverse_q + 1) * ub)
    return out


def cald_rankings(cls_cons, cls_count, labelled: Sequence[int]) -> Tuple[List[int], Dict[int, float]]:
    """``(sorted_indices, idx_to_jsdiv)`` of cald_ent.py:91-167.

    A frame's consistency is ``min(1.0, min over its matches)`` (``cls_cons`` holds 1.0 for a class without a match, so a
    frame without any stays at the reference's seed 1.0); ``sorted_indices`` is the stable ascending order over ALL frames.
    The divergence is computed for the frames with at least one match only, inserted in that order:
    ``q = softmax(the frame's matched-class histogram)`` in float64 over exactly ten slots, ``p = softmax(the labelled
    frames' class counts)``, and the two ``KLDivLoss(reduction='none')`` halves against ``log((p + q) / 2)``.

    The reference numbers the classes by first appearance among the labelled frames; softmax and the sums are
    permutation-invariant, so the merged label order is used here.  Difference kept on purpose: a class matched only
    outside the labelled set is counted in ``q`` here, where the reference's ``name_to_class`` lookup raises ``KeyError``."""
    cls_cons = np.asarray(cls_cons, dtype=np.float64)
    cls_count = np.asarray(cls_count).astype(np.int64)
    n, ncls = cls_count.shape
    if ncls > CALD_SLOTS:
        raise IndexError(f"cald_rankings: {ncls} classes, the reference's histogram has {CALD_SLOTS} slots")
    labelled = list(labelled)
    if not labelled:
        raise ValueError("cald_rankings: no labelled frame (the reference's labelled distribution is undefined)")
    cons = np.minimum(1.0, cls_cons.min(axis=1)) if n else np.zeros((0,))
    order = np.argsort(cons, kind="stable")
    sorted_indices = [int(i) for i in order]
    idx_list = [i for i in sorted_indices if cls_count[i].sum() > 0]
    hist = np.zeros((len(idx_list), CALD_SLOTS), dtype=np.float64)
    hist[:, :ncls] = cls_count[idx_list]
    lab = np.zeros((CALD_SLOTS,), dtype=np.int64)
    lab[:ncls] = cls_count[labelled].sum(axis=0)
    with torch.no_grad():
        # cald_ent.py:150-155: the same row once per labelled frame, averaged
        result = torch.tensor(np.mean(np.tile(lab, (len(labelled), 1)), axis=0)).unsqueeze(0)
        p = torch.nn.functional.softmax(result, -1)
        q = torch.nn.functional.softmax(torch.tensor(hist, dtype=torch.float64), -1)
        log_mean = ((p + q) / 2).log()
        kl = torch.nn.KLDivLoss(reduction="none")
        jsdiv = torch.sum(kl(log_mean, p.expand_as(q)), dim=1) / 2 + torch.sum(kl(log_mean, q), dim=1) / 2
    return sorted_indices, {int(i): float(jsdiv[k].item()) for k, i in enumerate(idx_list)}


# ------------------------------------------------------------------------------------------- the three files
def _write_atomic(path, mode, writer) -> None:
    """Rank 0 only, through a temporary file + ``os.replace``: a reader never sees a torn file."""
    if _rank() != 0:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, mode) as f:
        writer(f)
    os.replace(tmp, path)


def write_ranking(path, sorted_indices) -> None:
    """``CaldSelector.buffer_path``: a JSON list (cald_ent.py:94-95)."""
    _write_atomic(path, "w", lambda f: json.dump([int(i) for i in sorted_indices], f))


def write_jsdiv(path, idx_to_jsdiv) -> None:
    """``CaldSelector.jsdiv_path``: a pickled ``{frame: divergence}`` like the reference's ``idx_to_jsdiv.pkl``
    (cald_ent.py:166-167), or a JSON object when the name ends in ``.json``."""
    d = {int(k): float(v) for k, v in idx_to_jsdiv.items()}
    if str(path).endswith(".json"):
        _write_atomic(path, "w", lambda f: json.dump({str(k): v for k, v in d.items()}, f))
    else:
        _write_atomic(path, "wb", lambda f: pickle.dump(d, f))


def write_class_weights(path, weights) -> None:
    """``PPALSelector.class_weight_file``: a JSON object keyed by class name (ppal_unc.py:100-101)."""
    _write_atomic(path, "w", lambda f: json.dump({str(k): float(v) for k, v in weights.items()}, f))


# ------------------------------------------------------------------------------------------- whole pre-passes
def range_filter_of(infos, class_names):
    """``(class_range [ncls], origins [N,2])`` of the devkit's range rule for det3d infos: detection_cvpr_2019's ranges,
    measured from the ego origin, which in the lidar frame the boxes live in is ``ref_from_car``'s translation
    (nusc_common.py:399-417); infos without it measure from the lidar origin."""
    cr = np.array([NUSC_CLASS_RANGE[c] for c in class_names], np.float32)
    org = np.array([np.asarray(i["ref_from_car"], np.float64)[:2, 3] if "ref_from_car" in i else (0.0, 0.0)
                    for i in infos], np.float32).reshape(len(infos), 2)
    return cr, org


def _barrier():
    """Rank 0's files are complete before any rank replays them."""
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()


def run_ppal_prepass(detector, dataloader, device, infos, labelled, class_weight_file, class_names=None, alpha=3.0,
                     ub=2.0, range_filter=False, **kw) -> Dict[str, float]:
    """Sweep, match against the ground truth of ``infos``, write ``class_weight_file``; returns the weights."""
    class_names = head_class_names(detector) if class_names is None else list(class_names)
    refs = FrameRefs.from_infos(infos, class_names)
    if range_filter:
        kw["class_range"], kw["origins"] = range_filter_of(infos, class_names)
    m = sweep_matches(detector, dataloader, device, refs, ncls=len(class_names), **kw)
    weights = ppal_class_weights(m["cls_count"], m["cls_quality"], labelled, class_names, alpha, ub)
    write_class_weights(class_weight_file, weights)
    _barrier()
    return weights


def run_cald_prepass(detector, dataloader, device, num_frames, labelled, view, buffer_path, jsdiv_path, ncls=None, **kw):
    """Two sweeps: the plain one's detections are the reference boxes of the one over ``view``; writes ``buffer_path`` and
    ``jsdiv_path``; returns ``(sorted_indices, idx_to_jsdiv)``."""
    ncls = len(head_class_names(detector)) if ncls is None else int(ncls)
    saved = getattr(dataloader, "view", None)
    if hasattr(dataloader, "view"):
        dataloader.view = None
    try:
        refs = sweep_detections(detector, dataloader, device, num_frames)
    finally:
        if hasattr(dataloader, "view"):
            dataloader.view = saved
    m = sweep_matches(detector, dataloader, device, refs, view=view, ncls=ncls, **kw)
    ranking, jsdiv = cald_rankings(m["cls_cons"], m["cls_count"], labelled)
    write_ranking(buffer_path, ranking)
    write_jsdiv(jsdiv_path, jsdiv)
    _barrier()
    return ranking, jsdiv
