"""BEVFusion's camera-only detector family: ``LSSTransform -> GeneralizedResNet -> LSSFPN -> CenterHead``
(bevfusion/configs/nuscenes/det/centerhead/lssfpn/camera/256x704/swint/default.yaml).

Reference: bevfusion/mmdet3d/models/vtransforms/lss.py:13-78 (``LSSTransform`` on ``BaseTransform``, base.py:16-163),
backbones/resnet.py:12-40 (``GeneralizedResNet``), necks/lss.py:12-65 (``LSSFPN``), fusion_models/bevfusion.py:24-305.
The image encoder (Swin-T, ``GeneralizedLSSFPN``), the frustum / plan / pooling kernels, the depth softmax and
``CenterHead`` are this build's existing modules; new here are the BEV decoder's residual blocks (conv2 + bn2, then
shortcut + ReLU by ``al3d_add_relu_nhwc_f32``; with ``AL3D_RES=fused`` all four as one launch,
``al3d_conv3x3_res_nhwc_f16x3``), ``LSSFPN``'s bilinear tail (``al3d_upsample_bilinear_ac_nhwc_f32``) and the detector class.

All maps are channels-last.  The BEV map leaves the view transform as [x, y] -- the reference's own [H = x, W = y] -- and
the whole decoder keeps that orientation, so the reference's 2-D kernels load untransposed and ``CenterHead`` is built
with ``transpose_input=False``: no transposition pass anywhere.  Parameter names follow the reference
(``encoders.camera.{backbone,neck,vtransform}.*``, ``decoder.{backbone,neck}.*``, ``heads.object.*``), so its state dicts
load with ``strict=True``.
"""
import torch
from torch import nn

from .. import detector_ops as D
from .. import lib
from ..selector_ops import _dev, _ptr, _stream
from ..weight_cache import PackCache
from . import builder
from .bevfusion_camera import LSSViewTransform
from .conv_layers import FoldedConv
from .registry import BACKBONES, DETECTORS, NECKS


class BasicBlock(nn.Module):
    """The standard two-layer residual block.  A RESTATEMENT of a third-party class: the reference imports
    ``mmcv.cnn.resnet.BasicBlock`` (resnet.py:4), which is not in its tree; this is the block as torchvision and mmcv
    both define it -- conv1 (3x3, stride s, no bias), bn1, ReLU, conv2 (3x3), bn2, ``downsample`` on the shortcut, add,
    ReLU -- pinned by the tests to ``torch.nn`` modules assembled the same way, not to reference output.

    Launches: conv1 + bn1 + ReLU, the shortcut's 1x1 conv + BN and conv2 + bn2 on the dense conv dispatch, add + ReLU as
    ``detector_ops.add_relu_nhwc`` (``AL3D_RES=two-step``, the default: measured faster); with ``AL3D_RES=fused``
    under f16x3, and under the other arithmetics, conv2 + bn2 + add + ReLU go through ``detector_ops.conv3x3_res_nhwc``."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self._c1 = FoldedConv([(self.conv1, self.bn1)])
        self._sc = None if downsample is None else FoldedConv([(downsample[0], downsample[1])], relu=False)
        self._conv2 = PackCache()

    def forward(self, x):
        if self.training:
            raise RuntimeError("al3d BasicBlock implements the eval() path only")
        two_step = D.MATH == "f16x3" and D.RES == "two-step"

        def build():
            w, scale, shift = D.fold_conv_bn([(self.conv2, self.bn2)])
            w, scale = w.to(x.device), scale.to(x.device)
            w, scale = D.pack_dense(w, scale, 3, 1, 1) if two_step else D.pack_res3x3(w, scale)
            return w, scale, shift.to(x.device)
        w, scale, shift = self._conv2.get(x.device, (self.conv2, self.bn2), (D.MATH, D.DENSE, two_step), build)
        y = self._c1(x)
        identity = x if self._sc is None else self._sc(x)
        if two_step:
            y = D.conv2d_nhwc(y, w, scale, shift, 3, 1, 1, False)
            return D.add_relu_nhwc(y, identity, True, out=y)
        return D.conv3x3_res_nhwc(y, w, scale, shift, identity, relu=True)


def make_res_layer(inplanes, planes, blocks, stride=1):
    """mmcv's ``make_res_layer`` for ``BasicBlock`` (restated like the block): a 1x1 / stride-s conv + BN on the first
    block's shortcut when the stride or the channel count changes."""
    downsample = None
    if stride != 1 or inplanes != planes * BasicBlock.expansion:
        downsample = nn.Sequential(nn.Conv2d(inplanes, planes * BasicBlock.expansion, 1, stride=stride, bias=False),
                                   nn.BatchNorm2d(planes * BasicBlock.expansion))
    layers = [BasicBlock(inplanes, planes, stride, downsample)]
    layers += [BasicBlock(planes * BasicBlock.expansion, planes) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


@BACKBONES.register_module
class GeneralizedResNet(nn.ModuleList):
    """backbones/resnet.py:12-40: one ``make_res_layer`` stage per ``(num_blocks, out_channels, stride)``; keys
    ``{stage}.{block}.conv1.weight``, ``.bn1.*``, ``.conv2.weight``, ``.bn2.*``, ``.downsample.0.weight``,
    ``.downsample.1.*``.  forward(x channels-last [B,H,W,in_channels]) -> list of the stage outputs."""

    def __init__(self, in_channels, blocks):
        super().__init__()
        self.in_channels, self.blocks = in_channels, [tuple(b) for b in blocks]
        for num_blocks, out_channels, stride in self.blocks:
            self.append(make_res_layer(in_channels, out_channels, num_blocks, stride=stride))
            in_channels = out_channels

    def forward(self, x):
        outputs = []
        for stage in self:
            x = stage(x)
            outputs.append(x)
        return outputs


@NECKS.register_module
class LSSFPN(nn.Module):
    """necks/lss.py:12-65: ``cat([interpolate(x[in_indices[0]], size of x[in_indices[1]], bilinear, align_corners=True),
    x[in_indices[1]]])`` -> ``fuse`` (1x1 + BN + ReLU, 3x3 + BN + ReLU) -> ``upsample`` (x scale_factor bilinear,
    align_corners=True, 3x3 + BN + ReLU).  Keys ``fuse.{0,1,3,4}.*``, ``upsample.{1,2}.*``.  Channels-last maps in and
    out.  Upsample + concatenation: ``al3d_lss_upsample_cat_mode_f32``; the tail's resize:
    ``al3d_upsample_bilinear_ac_nhwc_f32``; the convolutions: the dense conv dispatch."""

    def __init__(self, in_indices, in_channels, out_channels, scale_factor=1):
        super().__init__()
        self.in_indices, self.in_channels = tuple(in_indices), tuple(in_channels)
        self.out_channels, self.scale_factor = out_channels, int(scale_factor)
        self.fuse = nn.Sequential(
            nn.Conv2d(in_channels[0] + in_channels[1], out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True),
            nn.Conv2d(out_channels, out_channels, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True))
        # the upsample + concatenation kernel writes the lateral map before the upsampled one, the reference concatenates
        # them the other way round: the 1x1 conv's weight columns are rotated by in_channels[0] when packed
        self._run = [FoldedConv([(self.fuse[0], self.fuse[1])], first=in_channels[0]), FoldedConv([(self.fuse[3], self.fuse[4])])]
        if self.scale_factor > 1:
            self.upsample = nn.Sequential(
                nn.Upsample(scale_factor=scale_factor, mode="bilinear", align_corners=True),
                nn.Conv2d(out_channels, out_channels, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True))
            self._run.append(FoldedConv([(self.upsample[1], self.upsample[2])]))

    def forward(self, x):
        if self.training:
            raise RuntimeError("al3d LSSFPN implements the eval() path only")
        x1, x2 = x[self.in_indices[0]], x[self.in_indices[1]]
        assert x1.shape[-1] == self.in_channels[0] and x2.shape[-1] == self.in_channels[1]
        if sum(self.in_channels) % 16 or x1.shape[-1] % 4 or x2.shape[-1] % 4:
            raise lib.Al3dError(f"LSSFPN: level channel counts {self.in_channels} must be multiples of 4 and sum to a "
                                "multiple of 16 (al3d_lss_upsample_cat_mode_f32, the matrix-core 1x1 convolution)")
        lat, src = _dev(x2, torch.float32, "lateral"), _dev(x1, torch.float32, "coarse level")
        cat = torch.empty((*lat.shape[:3], lat.shape[-1] + src.shape[-1]), dtype=torch.float32, device=lat.device)
        lib.call("al3d_lss_upsample_cat_mode_f32", _ptr(lat), _ptr(src), lat.shape[0], lat.shape[1], lat.shape[2], lat.shape[3],
                 src.shape[1], src.shape[2], src.shape[3], 1, _ptr(cat), _stream())
        y = self._run[1](self._run[0](cat))
        if self.scale_factor > 1:
            y = self._run[2](D.upsample_bilinear_ac_nhwc(y, (y.shape[1] * self.scale_factor, y.shape[2] * self.scale_factor)))
        return y


@NECKS.register_module
class LSSTransform(LSSViewTransform):
    """vtransforms/lss.py:13-78 + ``BaseTransform.forward`` (base.py:79-163): the plain Lift-Splat transform, no lidar
    points involved.  ``depthnet`` (1x1 with bias, in_channels -> D + C) on the dense conv dispatch, softmax over the D
    depth logits (``al3d_lss_depth_softmax_f32``), then the inherited frustum geometry, pooling plan and fused
    Lift-Splat pooling (the [B,N,D,fH,fW,C] product is never formed) and ``downsample``.  Registered with the NECKS: this
    build has no view-transform registry (the camera+lidar model constructs its transform directly) and adding one is
    outside this module; the detector below is the only place that builds it from a config.

    forward(img [B,N,fH,fW,in_channels] channels-last image features, camera_intrinsics / camera2lidar /
    img_aug_matrix [B,N,4,4], lidar_aug_matrix [B,4,4]) -> BEV map [B, nx0/ds, nx1/ds, C], [x, y] order."""

    def __init__(self, in_channels, out_channels, image_size, feature_size, xbound, ybound, zbound, dbound, downsample=1):
        super().__init__(out_channels, tuple(image_size), tuple(feature_size), list(xbound), list(ybound), list(zbound),
                         list(dbound), downsample)
        self.in_channels = in_channels
        self.depthnet = nn.Conv2d(in_channels, self.D + self.C, 1)
        self._dn = FoldedConv([(self.depthnet, None)], relu=False)

    def get_cam_feats(self, x):
        """x [B,N,fH,fW,Cin] -> (depth probabilities [B*N,D,fH,fW], context [B*N,fH,fW,C]); the reference's return value
        is their outer product [B,N,D,fH,fW,C] (lss.py:62-73)."""
        B, N, fH, fW, Cin = x.shape
        y = self._dn(x.reshape(B * N, fH, fW, Cin)).contiguous()
        depth = torch.empty((B * N, self.D, fH, fW), dtype=torch.float32, device=y.device)
        lib.call("al3d_lss_depth_softmax_f32", _ptr(y), B * N, fH, fW, self.D, y.shape[-1], _ptr(depth), _stream())
        return depth, y[..., self.D:self.D + self.C].contiguous()

    def forward(self, img, cam_intrinsic, camera2lidar, img_aug_matrix, lidar_aug_matrix, calib_key=None):
        B, N = img.shape[:2]
        depth, ctx = self.get_cam_feats(img)
        held = self.__dict__.get("_rows_cache")
        # the rows are a function of the calibration only: kept per calib_key, as DepthLSSTransform._calib_cached keeps its
        # own (that helper lives on the sibling class, which this module does not touch; one slot is all that is needed here)
        if calib_key is None or held is None or held[0] != calib_key:
            rows = self.geometry_rows(camera2lidar[..., :3, :3], camera2lidar[..., :3, 3], cam_intrinsic[..., :3, :3],
                                      img_aug_matrix[..., :3, :3], img_aug_matrix[..., :3, 3],
                                      extra_rots=lidar_aug_matrix[..., :3, :3], extra_trans=lidar_aug_matrix[..., :3, 3])
            held = (calib_key, rows)
            object.__setattr__(self, "_rows_cache", held)
        x = self.pool_lss(depth, ctx, held[1], B, N, calib_key=calib_key)
        for layer in self._ds:
            x = layer(x)
        return x


CAMERA_ONLY_KEYS = ("img", "camera_intrinsics", "camera2lidar", "img_aug_matrix", "lidar_aug_matrix")


@DETECTORS.register_module
class BEVFusionCameraOnly(nn.Module):
    """The camera-only model behind the det3d detector contract (same contract as ``BEVFusion.forward``).

    ``BEVFusionCameraOnly(camera=dict(backbone=..., neck=..., vtransform=...), decoder=dict(backbone=..., neck=...),
    bbox_head=<CenterHead cfg or None>, map_head=<BEVSegmentationHead cfg or None>)``;
    ``detector(example, return_loss=False, estimate=True)`` ->
    ``(list[dict(box3d_lidar, scores, label_preds, metadata)], [middle])`` with ``middle[-1]`` the decoder neck's map
    ([B, C, x, y]-shaped view) and its global average the embedding.  ``example``: the batch of
    ``CameraLidarSweepLoader`` / ``CameraLidarFileLoader``; its lidar keys are not read.  With a ``map_head``
    (``heads.map.*``, the reference's seg models) every output dict also holds ``masks_bev`` [K, X, Y] (probabilities),
    ``map_entropy`` [K] (mean binary entropy per class) and ``map_area`` [K] (cells above 0.5), and the plain
    ``return_loss=False`` call works without a ``bbox_head``."""

    def __init__(self, camera, decoder, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None, map_head=None):
        super().__init__()
        vt = camera["vtransform"]
        self.encoders = nn.ModuleDict(dict(camera=nn.ModuleDict(dict(
            backbone=builder.build_backbone(camera["backbone"]) if isinstance(camera["backbone"], dict) else camera["backbone"],
            neck=builder.build_neck(camera["neck"]) if isinstance(camera["neck"], dict) else camera["neck"],
            vtransform=builder.build_neck(dict(vt, type=vt.get("type", "LSSTransform"))) if isinstance(vt, dict) else vt))))
        self.decoder = nn.ModuleDict(dict(
            backbone=builder.build_backbone(decoder["backbone"]) if isinstance(decoder["backbone"], dict) else decoder["backbone"],
            neck=builder.build_neck(decoder["neck"]) if isinstance(decoder["neck"], dict) else decoder["neck"]))
        head = builder.build_head(bbox_head) if isinstance(bbox_head, dict) else bbox_head
        self.heads = nn.ModuleDict({} if head is None else dict(object=head))
        if map_head is not None:
            self.heads["map"] = builder.build_head(map_head) if isinstance(map_head, dict) else map_head
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.stage_ms = None

    @property
    def bbox_head(self):
        return self.heads["object"] if "object" in self.heads else None

    @property
    def map_head(self):
        return self.heads["map"] if "map" in self.heads else None

    def prepare(self, example):
        """No index work to run ahead: there is no sparse encoder."""
        return None

    def _run(self, example, timed=False):
        """-> (embedding [B,C], decoder map [B,X,Y,C], raw head predictions or None)."""
        cam = self.encoders["camera"]
        img = example["img"]
        B, N = img.shape[:2]
        marks = []

        def mark(name):
            if timed:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append((name, e))
        mark("start")
        feats = cam["backbone"](img.reshape(B * N, *img.shape[2:]))
        mark("camera backbone")
        fpn = cam["neck"](list(feats))
        fpn = fpn[0] if isinstance(fpn, (tuple, list)) else fpn
        mark("camera neck")
        bev = cam["vtransform"](fpn.view(B, N, *fpn.shape[1:]), example["camera_intrinsics"], example["camera2lidar"],
                                example["img_aug_matrix"], example["lidar_aug_matrix"], calib_key=example.get("calib_key"))
        mark("view transform (LSS)")
        dec = self.decoder["neck"](self.decoder["backbone"](bev))
        mark("decoder (GeneralizedResNet + LSSFPN)")
        emb = D.gap_nhwc(dec)
        mark("embedding")
        preds = None
        head = self.bbox_head
        if head is not None:
            preds = head(dec)
            if timed:
                head.get_bboxes(preds)                 # the decode is part of the stage's time
            mark(type(head).__name__)
        if timed:
            torch.cuda.synchronize()
            self.stage_ms = {b[0]: a[1].elapsed_time(b[1]) for a, b in zip(marks[:-1], marks[1:])}
        return emb, dec, preds

    def forward(self, example, return_loss=True, finetune=False, book=None, **kwargs):
        if return_loss:
            raise NotImplementedError("al3d implements the inference sweep, not training")
        missing = [k for k in CAMERA_ONLY_KEYS if k not in example]
        if missing:
            raise KeyError(f"BEVFusionCameraOnly: the example lacks the camera side {missing} (use CameraLidarSweepLoader)")
        from .detectors import NHWCFeature
        emb, dec, preds = self._run(example, timed=kwargs.get("timed", False))
        metas = example.get("metadata", None) or [None] * dec.shape[0]
        head, map_head = self.bbox_head, self.map_head
        if head is None:
            if map_head is None and not kwargs.get("estimate", False):
                raise RuntimeError("this detector was built without a bbox_head: only the estimate=True embedding sweep "
                                   "is available")
            out = [dict(metadata=m) for m in metas]
        else:
            out = head.predict(example, preds, self.test_cfg)
        if map_head is not None:
            prob, ent, area = map_head(dec, with_stats=True)
            for i, o in enumerate(out):
                o.update(masks_bev=prob[i], map_entropy=ent[i], map_area=area[i])
        if kwargs.get("estimate", False):
            return out, [NHWCFeature(dec, emb)]
        return out
