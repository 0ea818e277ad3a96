"""Voxel feature readers (reference det3d/models/readers/voxel_encoder.py:198-211, pillar_encoder.py:17-152)."""
import torch
from torch import nn

from .. import detector_ops as D
from .. import lib
from ..selector_ops import _ptr, _stream
from ..weight_cache import PackCache
from .registry import READERS


@READERS.register_module
class VoxelFeatureExtractorV3(nn.Module):
    """Mean of the points of each voxel.  ``forward(features [M,T,F], num_voxels [M])``
    like the reference; the device voxelizer already emits the mean, in which case the
    detector skips this module."""

    def __init__(self, num_input_features=4, norm_cfg=None, name="VoxelFeatureExtractorV3"):
        super().__init__()
        self.name = name
        self.num_input_features = num_input_features

    def forward(self, features, num_voxels, coors=None):
        if not features.is_cuda:
            raise lib.Al3dError("VoxelFeatureExtractorV3: device tensors required (no CPU fallback)")
        f = features[:, :, : self.num_input_features].contiguous().float()
        num = num_voxels.to(torch.int32).contiguous()
        m, t, c = f.shape
        out = torch.empty((m, c), dtype=torch.float32, device=f.device)
        lib.call("al3d_vfe_mean_f32", _ptr(f), _ptr(num), m, t, c, _ptr(out), _stream())
        return out


class PFNLayer(nn.Module):
    """One PFN layer's parameters (reference pillar_encoder.py:17-58): ``linear`` (no bias) + ``norm`` (BN1d).  The
    forward pass is the fused pillar kernel of ``PillarFeatureNet``; a layer that is not the last keeps half the units
    and concatenates them with their max over the pillar's slots."""

    def __init__(self, in_channels, out_channels, norm_cfg=None, last_layer=False):
        super().__init__()
        self.name = "PFNLayer"
        self.last_vfe = last_layer
        if not self.last_vfe:
            out_channels = out_channels // 2
        self.units = out_channels
        if norm_cfg is None:
            norm_cfg = dict(type="BN1d", eps=1e-3, momentum=0.01)
        self.norm_cfg = norm_cfg
        self.linear = nn.Linear(in_channels, self.units, bias=False)
        self.norm = nn.BatchNorm1d(self.units, eps=norm_cfg.get("eps", 1e-5), momentum=norm_cfg.get("momentum", 0.1))


@READERS.register_module
class PillarFeatureNet(nn.Module):
    """PointPillars pillar feature net (det3d/models/readers/pillar_encoder.py:61-152; BEVFusion's
    bevfusion/mmdet3d/models/backbones/pillar_encoder.py:85-182 under its keyword names ``in_channels``,
    ``feat_channels``, ``point_cloud_range``).  Same module tree and parameter names (``pfn_layers.<i>.linear.weight``,
    ``pfn_layers.<i>.norm.*``).

    ``forward(features [M,P,F], num_voxels [M], coors [M,4] (b,z,y,x))`` -> ``[M, C]`` from one launch of
    ``al3d_pillar_net_f32`` (csrc/pillars.hip): the padded slots take part in both max reductions as in the reference.
    Deviation: the reference ends in ``squeeze()``, which drops dimensions for M = 1 (and M = 0); this returns
    ``[M, C]`` for every M."""

    def __init__(self, num_input_features=4, num_filters=(64,), with_distance=False, voxel_size=(0.2, 0.2, 4),
                 pc_range=(0, -40, -3, 70.4, 40, 1), norm_cfg=None, in_channels=None, feat_channels=None,
                 point_cloud_range=None, name="PillarFeatureNet"):
        super().__init__()
        if in_channels is not None:
            num_input_features = in_channels
        if feat_channels is not None:
            num_filters = feat_channels
        if point_cloud_range is not None:
            pc_range = point_cloud_range
        self.name = name
        assert len(num_filters) > 0
        self.num_input = num_input_features
        nin = num_input_features + 5 + (1 if with_distance else 0)
        self._with_distance = with_distance
        filters = [nin] + list(num_filters)
        self.pfn_layers = nn.ModuleList([
            PFNLayer(filters[i], filters[i + 1], norm_cfg=norm_cfg, last_layer=i == len(filters) - 2)
            for i in range(len(filters) - 1)])
        self.vx, self.vy = voxel_size[0], voxel_size[1]
        self.x_offset = self.vx / 2 + pc_range[0]
        self.y_offset = self.vy / 2 + pc_range[1]
        self.out_channels = self.pfn_layers[-1].units
        self._packs = PackCache()

    def net(self, device):
        """The folded device weights (``detector_ops.PillarNet``), re-packed when a parameter or buffer changed."""
        if self.training:
            raise RuntimeError("al3d PillarFeatureNet implements the eval() sweep only")
        layers = [(p.linear, p.norm) for p in self.pfn_layers]
        return self._packs.get(device, [m for pair in layers for m in pair], None, lambda: D.PillarNet(
            layers, self.vx, self.vy, self.x_offset, self.y_offset, self._with_distance, device))      # fp32: one variant

    def forward(self, features, num_voxels, coors):
        if not features.is_cuda:
            raise lib.Al3dError("PillarFeatureNet: device tensors required (no CPU fallback)")
        return self.net(features.device).rows(features.float(), num_voxels, coors)


@READERS.register_module
class DynamicPillarFeatureNet(PillarFeatureNet):
    """``PillarFeatureNet`` over ALL points of every pillar, for the dynamic voxelizer (``max_points_in_voxel = -1`` /
    ``max_voxel_num = -1``): no cap per pillar or per frame, so the output is a function of the point set and the
    parameters alone.  Same constructor, module tree and parameter names: a PointPillars checkpoint loads with
    ``strict=True``.

    ``forward(points [N,F], point2voxel [N] (row or -1), mean [M,>=3], coors [M,4] (b,z,y,x))`` -> ``[M, C]`` from
    ``al3d_pillar_net_dynamic_f32`` (csrc/pillars_dyn.hip); ``mean`` is the voxelizer's ``feat`` (reduce = mean).
    Deviation from the hard reader, on purpose: there are no padded slots, so no ``relu(shift)`` row enters the max
    reductions -- a pillar that fills all its slots gets the hard reader's bits, a partly filled one can come out lower."""

    def __init__(self, *args, name="DynamicPillarFeatureNet", **kwargs):
        super().__init__(*args, name=name, **kwargs)

    def forward(self, points, point2voxel, mean, coors):
        if not points.is_cuda:
            raise lib.Al3dError("DynamicPillarFeatureNet: device tensors required (no CPU fallback)")
        return self.net(points.device).rows_dynamic(points.float(), point2voxel, mean, coors)
