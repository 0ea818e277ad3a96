"""Detector graphs (reference det3d/models/detectors/{single_stage,voxelnet}.py).

Call contract kept: ``detector(example, return_loss=False, estimate=True)`` returns
``(list[dict(box3d_lidar, scores, label_preds, metadata)], middle)`` with ``middle[-1]`` the
neck output (voxelnet.py:73-81,115-116).  Activations are channels-last in this build, so
``middle[-1]`` is wrapped in ``NHWCFeature`` whose ``mean(-1).mean(-1)`` -- the expression the
selectors apply to it (feature_selector.py:68-71) -- runs the device GAP kernel.
"""
import torch
from torch import nn

from .. import detector_ops as D
from . import builder
from .registry import DETECTORS


class NHWCFeature:
    """A ``[B,C,H,W]``-shaped view of an NHWC buffer for the selectors' embedding tap."""

    def __init__(self, nhwc, embedding=None, pair=False):
        self._nhwc, self._pair = nhwc, pair   # pair: the buffer holds pair pixels (csrc/sp_rows.h), converted on access
        self._emb = embedding           # [B,C] global average the neck already produced (fused GAP), or None
        B, H, W, C = nhwc.shape
        self.shape = torch.Size((B, C, H, W))
        self.device = nhwc.device
        self._w_reduced = False

    @property
    def nhwc(self):
        if self._pair:
            C = self._nhwc.shape[-1]
            self._nhwc, self._pair = D.rows_convert(self._nhwc.view(-1, C), False).view_as(self._nhwc), False
        return self._nhwc

    def mean(self, dim=-1):
        if not self._w_reduced:
            r = NHWCFeature.__new__(NHWCFeature)
            r._nhwc, r._pair, r.shape, r.device, r._w_reduced, r._emb = \
                self._nhwc, self._pair, self.shape[:3], self.device, True, self._emb
            return r
        if self._emb is not None:
            return self._emb                   # emitted by the neck's deblock launches (al3d_*_gap)
        return D.gap_nhwc(self.nhwc)          # mean over W, then over H, in one kernel

    def nchw(self):
        return self.nhwc.permute(0, 3, 1, 2)


@DETECTORS.register_module
class SingleStageDetector(nn.Module):
    def __init__(self, reader, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None):
        super().__init__()
        self.reader = builder.build_reader(reader)
        self.backbone = builder.build_backbone(backbone)
        if neck is not None:
            self.neck = builder.build_neck(neck)
        # bbox_head=None: embedding-only graph (BEVFusion lidar branch, models/bevfusion_compat.py)
        self.bbox_head = builder.build_head(bbox_head) if bbox_head is not None else None
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg

    @property
    def with_neck(self):
        return hasattr(self, "neck") and self.neck is not None


@DETECTORS.register_module
class FPNVoxelNet(SingleStageDetector):
    # may the encoder hand this detector's own neck its last level as rows (detector_ops.BevRows)?  False where something
    # else reads the encoder's dense map (BEVFusion's fuser)
    neck_rows = True

    def _neck_rows(self):
        """The rows hand-over is possible for this encoder / neck pair under the current arithmetic and knobs."""
        import inspect
        return bool(self.neck_rows and self.with_neck and hasattr(self.neck, "rows_input_ok") and
                    "neck_rows" in inspect.signature(self.backbone.forward).parameters and self.neck.rows_input_ok())

    def _input_features(self, data):
        """The encoder's input rows.  A mean reader's (``mean_reader``, VoxelFeatureExtractorV3) output is what the device
        voxelizer already emits as ``voxel_features``: that shortcut is taken only for such a reader.  Any other reader
        runs on the padded point slots, which the loader yields under ``with_points=True``."""
        if getattr(self.reader, "mean_reader", False) and data.get("mean_features") is not None:
            return data["mean_features"]
        if data.get("features") is None or data.get("num_voxels") is None:
            raise RuntimeError(f"{type(self).__name__} with a {type(self.reader).__name__} reader needs the padded point "
                               "slots (voxels, num_points): build the loader with with_points=True")
        return self.reader(data["features"], data["num_voxels"])

    @staticmethod
    def _map_and_middle(out):
        """An encoder returns (map, middle) -- the FPN encoder -- or, like the reference's SpMiddleFHD /
        SpMiddleResNetFHD, the map alone: ``middle`` then starts empty (the neck's output is still appended)."""
        if isinstance(out, tuple):
            return out[0], out[1]
        return out, []

    def extract_feat(self, data):
        input_features = self._input_features(data)
        x, middle = self._map_and_middle(self.backbone(input_features, data["coors"], data["batch_size"],
                                                       data["input_shape"], **self._cap_kw(data.get("voxel_cap", 0))))
        if self.with_neck:
            x = self.neck(x)
            middle.append(NHWCFeature(x, getattr(self.neck, "embedding", None)))
        return x, middle

    # The forward pass is exposed in two halves so that the sweep can run the sparse half of batch
    # i+1 (voxel features -> sparse encoder -> dense BEV; latency-bound gathers) on one HIP stream
    # while the dense half of batch i (neck + head + decode; matrix-core bound) runs on another.
    def _cap_kw(self, cap):
        """``voxel_cap`` of a device-voxelized example (frames concatenated in order, at most that many rows each) as the
        sparse encoder's ``frame_rows_max`` promise, for encoders that take it."""
        import inspect
        if cap and "frame_rows_max" in inspect.signature(self.backbone.forward).parameters:
            return {"frame_rows_max": int(cap)}
        return {}

    def prepare(self, example):
        """Index work of a batch (sparse-conv rulebook); needs ``coordinates`` only, so the sweep runs
        it one batch ahead on a side stream.  Pass the result as ``book=`` to forward / sparse_stage."""
        if not hasattr(self.backbone, "rulebook_for"):
            return None
        kw = self._cap_kw(example.get("voxel_cap", 0))
        if self._neck_rows():
            kw["neck_rows"] = True
        return self.backbone.rulebook_for(example["coordinates"], len(example["num_voxels"]), example["shape"][0], **kw)

    def sparse_stage(self, example, book=None, neck_rows=False):
        """-> (dense BEV map, middle).  ``neck_rows=True`` (the result goes to ``dense_stage``): the map may come as a
        ``detector_ops.BevRows`` for the neck's first conv to read in place."""
        rows_kw = {"neck_rows": True} if neck_rows and self._neck_rows() else {}
        num_voxels = example["num_voxels"]
        data = dict(features=example.get("voxels"), num_voxels=example.get("num_points"),
                    mean_features=example.get("voxel_features"), coors=example["coordinates"],
                    batch_size=len(num_voxels), input_shape=example["shape"][0], voxel_cap=example.get("voxel_cap", 0))
        input_features = self._input_features(data)
        if book is not None:
            return self._map_and_middle(self.backbone(input_features, data["coors"], data["batch_size"],
                                                      data["input_shape"], book=book, **rows_kw))
        return self._map_and_middle(self.backbone(input_features, data["coors"], data["batch_size"], data["input_shape"],
                                                  **self._cap_kw(data["voxel_cap"]), **rows_kw))

    def dense_stage(self, example, x, middle, finetune=False, **kwargs):
        pair = False
        if self.with_neck:
            want = self.bbox_head is not None and hasattr(self.bbox_head, "accepts_pair") and \
                self.bbox_head.accepts_pair(x.device)
            import inspect
            want = want and "out_pair" in inspect.signature(self.neck.forward).parameters
            x = self.neck(x, out_pair=True) if want else self.neck(x)
            pair = bool(want and getattr(self.neck, "last_out_pair", False))
            middle.append(NHWCFeature(x, getattr(self.neck, "embedding", None), pair=pair))
        return self._head_stage(example, x, middle, pair, finetune=finetune, **kwargs)

    def _head_stage(self, example, x, middle, pair, finetune=False, **kwargs):
        if self.bbox_head is None:
            if not kwargs.get("estimate", False):
                raise RuntimeError("this detector was built without a bbox_head: only the estimate=True "
                                   "embedding sweep is available")
            return [dict(metadata=m) for m in example.get("metadata", [None] * x.shape[0])], middle
        preds = self.bbox_head(x, finetune=finetune, in_pair=True) if pair else self.bbox_head(x, finetune=finetune)
        if kwargs.get("get_preds", False):
            return preds
        out = self.bbox_head.predict(example, preds, self.test_cfg)
        if kwargs.get("estimate", False):
            return out, middle
        return out

    def forward(self, example, return_loss=True, finetune=False, **kwargs):
        if return_loss:
            raise NotImplementedError("al3d implements the inference sweep, not training")
        x, middle = self.sparse_stage(example, book=kwargs.pop("book", None), neck_rows=True)
        return self.dense_stage(example, x, middle, finetune=finetune, **kwargs)


@DETECTORS.register_module
class VoxelNet(FPNVoxelNet):
    """Same graph; ``forward`` returns detections only (voxelnet.py:8-55).  The reference's ``VoxelNet.extract_feat``
    calls its reader with two arguments (voxelnet.py:24), which its own ``VoxelFeatureExtractor`` -- three positional
    parameters -- does not accept; here every reader takes ``coors=None``, so SECOND's learned reader runs under this
    detector too."""

    def forward(self, example, return_loss=True, **kwargs):
        kwargs.pop("estimate", None)
        return super().forward(example, return_loss=return_loss, **kwargs)


@DETECTORS.register_module
class PointPillars(FPNVoxelNet):
    """PointPillars (det3d/models/detectors/point_pillars.py; BEVFusion's PointPillarsEncoder,
    bevfusion/mmdet3d/models/backbones/pillar_encoder.py:243-258): ``PillarFeatureNet`` reader, ``PointPillarsScatter``
    backbone, dense neck, optional head.  Same call contract as ``FPNVoxelNet``; the example must carry the padded
    point slots (``voxels``, ``num_points``: the loaders' ``with_points=True``).  With a ``DynamicPillarFeatureNet``
    reader it carries ``points``, ``point2voxel`` and ``voxel_features`` of the dynamic voxelizer instead (the loaders'
    ``keep_points=True``) and every point of every pillar counts (``al3d_pillar_net_dynamic_f32``, canvas form).

    ``sparse_stage`` runs the reader and the scatter as ONE launch (``al3d_pillar_net_scatter_f32``): the pillar rows
    go straight into the zeroed NHWC canvas.  There is no rulebook (``prepare`` returns None).  The dense kernels take
    maps below 2^31 elements; a larger canvas (512 x 512 x 64 at batch >= 128) runs the neck in frame chunks, which
    gives the same bits as running the chunks as batches of their own."""

    DENSE_LIMIT = 1 << 31

    def prepare(self, example):
        return None

    def extract_feat(self, data):
        """det3d's point_pillars.py:23-39 keys (features, num_voxels, coors, batch_size, input_shape) -> (canvas, [])."""
        nx, ny = int(data["input_shape"][0]), int(data["input_shape"][1])
        if self._dynamic():
            # the dynamic reader's keys: points, point2voxel, mean_features (the voxelizer's feat), coors
            self._need_points(data.get("points"), data.get("point2voxel"), data.get("mean_features"))
            net = self.reader.net(data["points"].device)
            x = net.canvas_dynamic(data["points"], data["point2voxel"], data["mean_features"], data["coors"],
                                   int(data["batch_size"]), ny, nx, check=False)
        else:
            net = self.reader.net(data["features"].device)
            x = net.canvas(data["features"].float(), data["num_voxels"], data["coors"], int(data["batch_size"]), ny, nx)
        middle = []
        if self.with_neck:
            x = self.neck(x)
            middle.append(NHWCFeature(x, getattr(self.neck, "embedding", None)))
        return x, middle

    def _dynamic(self):
        from .readers import DynamicPillarFeatureNet
        return isinstance(self.reader, DynamicPillarFeatureNet)

    @staticmethod
    def _need_points(points, point2voxel, mean):
        if points is None or point2voxel is None or mean is None:
            raise RuntimeError("PointPillars with DynamicPillarFeatureNet needs the batch's points, point2voxel and voxel "
                               "means: build the loader with keep_points=True on a dynamic voxel_generator "
                               "(max_points_in_voxel = -1, max_voxel_num = -1)")

    def sparse_stage(self, example, book=None, neck_rows=False):       # the canvas is dense: neck_rows does not apply
        if self._dynamic():
            pts, p2v, mean = example.get("points"), example.get("point2voxel"), example.get("voxel_features")
            self._need_points(pts, p2v, mean)
            nx, ny = int(example["shape"][0][0]), int(example["shape"][0][1])
            # one fused call; point2voxel was validated with the voxelizer's status word at the loader's host sync
            x = self.reader.net(pts.device).canvas_dynamic(pts, p2v, mean, example["coordinates"],
                                                           len(example["num_voxels"]), ny, nx, check=False)
            return x, []
        voxels = example.get("voxels")
        if voxels is None:
            raise RuntimeError("PointPillars needs the padded point slots: build the loader with with_points=True")
        nx, ny = int(example["shape"][0][0]), int(example["shape"][0][1])
        net = self.reader.net(voxels.device)
        x = net.canvas(voxels, example["num_points"], example["coordinates"], len(example["num_voxels"]), ny, nx)
        return x, []

    def dense_stage(self, example, x, middle, finetune=False, **kwargs):
        B, H, W, C = x.shape
        if not self.with_neck or B * H * W * C < self.DENSE_LIMIT:
            return super().dense_stage(example, x, middle, finetune=finetune, **kwargs)
        n = max(1, (self.DENSE_LIMIT - 1) // (H * W * C))
        outs, embs = [], []
        for s in range(0, B, n):
            outs.append(self.neck(x[s:s + n]))
            embs.append(getattr(self.neck, "embedding", None))
        y = torch.cat(outs)
        emb = torch.cat(embs) if all(e is not None for e in embs) else None
        middle.append(NHWCFeature(y, emb))
        return self._head_stage(example, y, middle, False, finetune=finetune, **kwargs)
