"""BEVFusion's BEV map segmentation head (bevfusion/mmdet3d/models/heads/segm/vanilla.py:47-138), selected by
configs/nuscenes/seg/default.yaml under ``heads.map``: ``BEVGridTransform`` (a bilinear resample of the decoder map
onto the map grid), two 3x3 Conv + BN + ReLU, a 1x1 Conv with bias, sigmoid.  Eval path only.

The resample is ``al3d_bev_grid_resample_nhwc_f32`` on host-built index / weight tables, the two 3x3 layers run on the
dense conv dispatch, the last layer with the sigmoid is ``al3d_seg_classify_f32``, which also returns per frame and
class the summed binary entropy and the count of pixels above 0.5 (what an acquisition function consumes; the reference
has no such output).  Maps are channels-last; parameter names are the reference's (``classifier.{0,1,3,4,6}.*``), so its
state dicts load with ``strict=True``.
"""
import torch
from torch import nn

from .. import detector_ops as D
from .. import lib
from .conv_layers import FoldedConv
from .registry import HEADS


class BEVGridTransform(nn.Module):
    """vanilla.py:47-87.  ``input_scope`` / ``output_scope``: per axis ``(min, max, step)`` of the map it receives and of the
    grid it returns; axis 0 is the map's first spatial axis (x in the reference's [x, y] maps).

    forward(x [B, h, w, C] channels-last) -> [B, H, W, C].  ``transposed=True``: x is stored [y, x] (its rows run along
    scope 1); the result is still [B, X, Y, C] -- the kernel writes it transposed, there is no pass of its own."""

    def __init__(self, *, input_scope, output_scope, prescale_factor=1):
        super().__init__()
        if prescale_factor != 1:
            raise NotImplementedError("al3d BEVGridTransform: prescale_factor != 1 is not implemented (no shipped config sets it)")
        self.input_scope = [tuple(float(v) for v in s) for s in input_scope]
        self.output_scope = [tuple(float(v) for v in s) for s in output_scope]
        self.prescale_factor = prescale_factor
        if len(self.input_scope) != 2 or len(self.output_scope) != 2:
            raise ValueError("BEVGridTransform: two axes expected")

    def forward(self, x, transposed=False):
        if transposed:
            return D.bev_grid_resample_nhwc(x, self.input_scope[::-1], self.output_scope[::-1], out_hw_swapped=True)
        return D.bev_grid_resample_nhwc(x, self.input_scope, self.output_scope)


@HEADS.register_module
class BEVSegmentationHead(nn.Module):
    """vanilla.py:90-138 with the reference's constructor arguments.  ``loss`` is kept for the configs' sake (the losses
    belong to training).  ``transpose_input=True``: the incoming map is stored [y, x] (this build's lidar neck); the
    output is the same [B, K, X, Y] as the plain head gives on the transposed map.

    forward(x) -> probabilities [B, K, X, Y]; forward(x, with_stats=True) -> (probabilities, mean binary entropy [B, K],
    area [B, K] int32: the cells with p > 0.5).  x: a channels-last map [B, h, w, in_channels] or a list whose first entry
    is one."""

    def __init__(self, in_channels, grid_transform, classes, loss, transpose_input=False):
        super().__init__()
        if in_channels % 32:
            raise lib.Al3dError(f"BEVSegmentationHead: in_channels={in_channels} must be a multiple of 32 (the dense conv "
                                "kernels' output tile)")
        if not 1 <= len(classes) <= 16:
            raise lib.Al3dError(f"BEVSegmentationHead: {len(classes)} classes; al3d_seg_classify_f32 serves 1 to 16")
        self.in_channels, self.classes, self.loss = in_channels, list(classes), loss
        self.transpose_input = bool(transpose_input)
        self.transform = BEVGridTransform(**grid_transform)
        self.classifier = nn.Sequential(
            nn.Conv2d(in_channels, in_channels, 3, padding=1, bias=False), nn.BatchNorm2d(in_channels), nn.ReLU(True),
            nn.Conv2d(in_channels, in_channels, 3, padding=1, bias=False), nn.BatchNorm2d(in_channels), nn.ReLU(True),
            nn.Conv2d(in_channels, len(classes), 1))
        self._run = [FoldedConv([(self.classifier[0], self.classifier[1])]), FoldedConv([(self.classifier[3], self.classifier[4])])]

    def forward(self, x, target=None, with_stats=False):
        if self.training:
            raise RuntimeError("al3d BEVSegmentationHead implements the eval() path only")
        if isinstance(x, (list, tuple)):
            x = x[0]
        if x.dim() != 4 or x.shape[-1] != self.in_channels:
            raise lib.Al3dError(f"BEVSegmentationHead: expected a channels-last map [B, h, w, {self.in_channels}], got "
                                f"{tuple(x.shape)}")
        y = self.transform(x, transposed=self.transpose_input)
        y = self._run[1](self._run[0](y))
        last = self.classifier[6]
        w = last.weight.detach().reshape(len(self.classes), self.in_channels)
        out = D.seg_classify(y, w, last.bias.detach(), with_stats=with_stats)
        if not with_stats:
            return out
        prob, ent, area = out
        return prob, ent / float(prob.shape[2] * prob.shape[3]), area
