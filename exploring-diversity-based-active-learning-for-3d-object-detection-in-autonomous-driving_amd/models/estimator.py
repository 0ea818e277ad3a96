"""The box-wise IoU estimator (reference det3d/models/detectors/estimator.py:22-105,155-274, the ``ESTIMATORS``-registered
class; its inference call is active_trainer.py:441-443) and the wrapper that puts it behind a detector.

A small PointNet that runs after the detector: for every predicted box it reads the lidar points in the box's doubled BEV
footprint and own height, and predicts the box's IoU with the ground truth.  The predicted IoU replaces the box's score;
boxes without a point are dropped.  Parameter names match the reference (``iou_estimator.{0,1,3,4,6,7}.*``,
``iou_head.{0,1,3,4,6}.*``), so its checkpoints load with ``strict=True``.  Everything runs in ``csrc/estimator.hip`` on
the raw NMS buffers; the BatchNorms are folded into the linears on the host, once per set of weights.

Parity quirks kept: the footprint is rotated clockwise for a positive angle and the point features
counter-clockwise, and the angle is column 6 of the box (``box[:, :7][:, -1]``), whatever the box's width.

Differs on purpose: a frame in which no box survives comes back with zero detections (the reference's ``torch.stack([])``
raises); ``example["middle"]`` and ``dim_feat`` are accepted and unused (the reference's feature interpolation is
commented out); ``return_loss=True`` raises ``NotImplementedError``."""
import torch
from torch import nn

from .. import selector_ops as ops
from ..lib import Al3dError
from ..weight_cache import PackCache
from .bbox_heads import LazyDetections, pack_detections
from .registry import ESTIMATORS

ROT_COL = 6         # box3d_lidar[:, :7][:, -1] (estimator.py:199-204)


def fold_linear_bn(linear, bn=None):
    """``Linear -> eval BatchNorm1d`` as one affine map, folded in float64: ``(W * s[:, None], (b - mean) * s + beta)``
    with ``s = gamma / sqrt(var + eps)``, rounded to float32 once."""
    w = linear.weight.detach().double()
    b = linear.bias.detach().double() if linear.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64,
                                                                                   device=w.device)
    if bn is not None:
        s = torch.rsqrt(bn.running_var.detach().double() + bn.eps)
        if bn.weight is not None:
            s = s * bn.weight.detach().double()
        b = (b - bn.running_mean.detach().double()) * s
        if bn.bias is not None:
            b = b + bn.bias.detach().double()
        w = w * s[:, None]
    return w.float(), b.float()


class RescoredDetections(LazyDetections):
    """``LazyDetections`` over the estimator's compacted buffers.  The kernel's status word travels to the host with the
    counts, when the dictionaries are first read; ``frame_entropy`` and the other device-side readers stay free of any
    synchronisation (a refused batch has zero counts there)."""

    def __init__(self, *args, status=None, **kw):
        super().__init__(*args, **kw)
        self._status = status

    def _materialize(self):
        if self._list is None:
            out = super()._materialize()
            if self._status is not None:
                ops.estimator_status_check(self._status.item())
            return out
        return self._list


def frame_points(example, batch):
    """``(points [P,F] f32, point_offsets [B+1] i64)`` of an example: this package's ``points`` + ``point_offsets``, or
    the reference's ``[P, 1+F]`` tensor with the batch index in column 0 (frames need not be sorted there)."""
    pts = example["points"]
    off = example.get("point_offsets")
    if off is not None:
        return pts.float().contiguous(), off.to(torch.int64)
    idx = pts[:, 0].long()
    order = torch.argsort(idx, stable=True)
    n = torch.bincount(idx, minlength=batch)[:batch]
    off = torch.zeros((batch + 1,), dtype=torch.int64, device=pts.device)
    off[1:] = torch.cumsum(n, 0)
    return pts[order][:, 1:].float().contiguous(), off


@ESTIMATORS.register_module
class Estimator(nn.Module):
    def __init__(self, tasks, dim_feat=0):
        super().__init__()
        self.dim_feat = dim_feat
        self.num_tasks = len(tasks)
        self.num_classes = sum(len(t["class_names"]) for t in tasks)
        if not 1 <= self.num_classes <= ops.EST_MAX_CLASSES:
            raise Al3dError(f"Estimator: {self.num_classes} classes, the kernel takes 1..{ops.EST_MAX_CLASSES}")

        def mlp(dims, last_plain=False):
            layers = []
            for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
                layers.append(nn.Linear(a, b))
                if not (last_plain and i == len(dims) - 2):
                    layers += [nn.BatchNorm1d(b), nn.ReLU(True)]
            return nn.Sequential(*layers)

        self.iou_estimator = mlp([9 + self.num_classes, 32, 64, 128])
        self.iou_head = mlp([128, 256, 64, 1], last_plain=True)
        self._packs = PackCache()

    def _sources(self):
        return [m for seq in (self.iou_estimator, self.iou_head) for m in seq if not isinstance(m, nn.ReLU)]

    def _pack(self, device):
        e, h = self.iou_estimator, self.iou_head
        parts = []
        for lin, bn in ((e[0], e[1]), (e[3], e[4]), (e[6], e[7])):
            w, b = fold_linear_bn(lin, bn)
            parts += [w.reshape(-1), b]                     # [out][in]: a lane holds one output's row
        for lin, bn in ((h[0], h[1]), (h[3], h[4])):
            w, b = fold_linear_bn(lin, bn)
            parts += [w.t().contiguous().reshape(-1), b]    # [in][out]: the lanes read consecutive outputs
        w, b = fold_linear_bn(h[6])
        parts += [w.reshape(-1), b]
        return torch.cat([p.to(device) for p in parts]).contiguous()

    def packed_weights(self, device):
        return self._packs.get(device, self._sources(), build=lambda: self._pack(device))

    def forward(self, example, return_loss=False, **kwargs):
        if return_loss:
            raise NotImplementedError("al3d implements the inference sweep, not training")
        if self.training:
            raise Al3dError("Estimator: eval() only (the BatchNorms are folded into the linears)")
        preds = example["preds"]
        lazy = isinstance(preds, LazyDetections)
        if lazy:
            boxes, scores, labels, counts, done, meta = preds._raw
            torch.cuda.current_stream(boxes.device).wait_event(done)
        else:
            preds = list(preds)
            if not preds:
                return []
            boxes, scores, labels, counts = pack_detections(preds)
            meta = [p.get("metadata") for p in preds]
        points, off = frame_points(example, boxes.shape[0])
        # check=False: nothing here waits for the device; the status word is read where the counts are
        res = ops.estimate_boxes(boxes, labels, counts, points, off, self.packed_weights(boxes.device), self.num_classes,
                                 rot_col=ROT_COL, check=False)
        finished = torch.cuda.Event()
        finished.record(torch.cuda.current_stream(boxes.device))
        out = RescoredDetections(res["boxes"], res["scores"], res["labels"], res["counts"], finished, meta,
                                 status=res["status"])
        if lazy:
            example["preds"] = out
            return out
        example["preds"] = list(out)
        return example["preds"]


class WithEstimator(nn.Module):
    """A detector whose predictions come back rescored by an ``Estimator`` (active_trainer.py:441-443: ``preds =
    model(example); example["preds"] = preds; estimator(example)``), behind the detector's own call contract:
    ``forward(..., estimate=True) -> (preds, middle)``, ``prepare``, ``sparse_stage`` / ``dense_stage``.  The examples it is
    fed must carry their points (``DeviceSweepLoader(keep_points=True)``, ``FileSweepLoader``)."""

    def __init__(self, detector, estimator):
        super().__init__()
        self.detector = detector
        self.estimator = estimator

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name in ("detector", "estimator"):
                raise
            return getattr(super().__getattr__("detector"), name)     # bbox_head, backbone, test_cfg, ...

    def _rescore(self, example, out, estimate):
        estimate = estimate and isinstance(out, tuple)      # VoxelNet.forward returns the detections alone
        preds, middle = out if estimate else (out, None)
        if "points" not in example:
            raise Al3dError("WithEstimator: the example carries no points (DeviceSweepLoader(keep_points=True))")
        ex = dict(example, preds=preds, middle=middle)
        preds = self.estimator(ex, return_loss=False)
        return (preds, middle) if estimate else preds

    def prepare(self, example):
        return self.detector.prepare(example)

    def sparse_stage(self, example, book=None, neck_rows=False):
        import inspect
        kw = {"neck_rows": neck_rows} if "neck_rows" in inspect.signature(self.detector.sparse_stage).parameters else {}
        return self.detector.sparse_stage(example, book=book, **kw)

    def dense_stage(self, example, x, middle, **kwargs):
        if kwargs.get("get_preds", False):
            return self.detector.dense_stage(example, x, middle, **kwargs)
        return self._rescore(example, self.detector.dense_stage(example, x, middle, **kwargs),
                             kwargs.get("estimate", False))

    def forward(self, example, return_loss=True, **kwargs):
        if return_loss:
            raise NotImplementedError("al3d implements the inference sweep, not training")
        if kwargs.get("get_preds", False):
            return self.detector(example, return_loss=False, **kwargs)
        return self._rescore(example, self.detector(example, return_loss=False, **kwargs), kwargs.get("estimate", False))
