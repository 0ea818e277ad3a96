"""Voxel feature readers (reference det3d/models/readers/voxel_encoder.py:13-235, pillar_encoder.py:17-152).

Every reader says what it needs from the loader in a class attribute: ``needs_point_slots`` (the padded point slots
``voxels`` / ``num_points``: the loaders' ``with_points=True``) and ``mean_reader`` (its output IS the voxelizer's mean,
so the detector may take the voxelizer's ``voxel_features`` instead of running it)."""
import torch
from torch import nn

from .. import detector_ops as D
from .. import lib
from ..selector_ops import _ptr, _stream
from ..weight_cache import PackCache
from .registry import READERS


def needs_point_slots(reader_cfg):
    """Does the reader a config names (``model.reader``) read the padded point slots?  What the tools hand the loaders
    as ``with_points``; a missing or unknown reader gives False (building the model reports an unknown name)."""
    cls = READERS.get((reader_cfg or {}).get("type")) if (reader_cfg or {}).get("type") else None
    return bool(getattr(cls, "needs_point_slots", False))


@READERS.register_module
class VoxelFeatureExtractorV3(nn.Module):
    """Mean of the points of each voxel.  ``forward(features [M,T,F], num_voxels [M])``
    like the reference; the device voxelizer already emits the mean, in which case the
    detector skips this module."""

    needs_point_slots = False
    mean_reader = True

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

    needs_point_slots = True
    mean_reader = False

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

    needs_point_slots = False            # it reads the dynamic voxelizer's points (the loaders' keep_points=True)

    def __init__(self, *args, name="DynamicPillarFeatureNet", **kwargs):
        super().__init__(*args, name=name, **kwargs)

    def forward(self, points, point2voxel, mean, coors):
        if not points.is_cuda:
            raise lib.Al3dError("DynamicPillarFeatureNet: device tensors required (no CPU fallback)")
        return self.net(points.device).rows_dynamic(points.float(), point2voxel, mean, coors)


# ------------------------------------------------------------------ det3d's learned VFE readers (SECOND)
class Empty(nn.Module):
    """The reference's stand-in for BatchNorm1d under ``use_norm=False`` (det3d/models/utils/misc.py): no parameters."""

    def __init__(self, *args, **kwargs):
        super().__init__()

    def forward(self, x):
        return x


def _vfe_linear_norm(cin, cout, use_norm):
    """(linear, norm) as voxel_encoder.py:19-26 builds them: bias-free linear + BN1d(eps 1e-3, momentum 0.01), or a linear
    with bias and no norm."""
    if use_norm:
        return nn.Linear(cin, cout, bias=False), nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01)
    return nn.Linear(cin, cout, bias=True), Empty(cout)


@READERS.register_module
class VFELayer(nn.Module):
    """One VFE layer's parameters (reference voxel_encoder.py:13-42): ``linear`` + ``norm`` with ``out_channels // 2``
    units; its output is [pointwise, max over the voxel's slots].  The forward pass is the fused kernel of
    ``VoxelFeatureExtractor`` / ``VoxelFeatureExtractorV2`` (csrc/vfe.hip); on its own the layer has none."""

    def __init__(self, in_channels, out_channels, use_norm=True, name="vfe"):
        super().__init__()
        self.name = name
        self.units = int(out_channels / 2)
        self.linear, self.norm = _vfe_linear_norm(in_channels, self.units, use_norm)

    def forward(self, inputs):
        raise NotImplementedError("al3d VFELayer holds parameters only: the layers run fused inside "
                                  "VoxelFeatureExtractor / VoxelFeatureExtractorV2 (al3d_vfe_net_f32)")


class _VFEBase(nn.Module):
    """Shared forward of the two learned readers: one ``al3d_vfe_net_f32`` launch on the padded point slots."""

    needs_point_slots = True
    mean_reader = False

    def _layers(self):
        raise NotImplementedError

    def net(self, device):
        """The folded device weights (``detector_ops.VfeNet``), re-packed when a parameter or buffer changed."""
        if self.training:
            raise RuntimeError(f"al3d {type(self).__name__} implements the eval() sweep only")
        layers = self._layers()
        return self._packs.get(device, [m for pair in layers for m in pair], None,
                               lambda: D.VfeNet(layers, self._with_distance, device))      # fp32: one variant

    def forward(self, features, num_voxels, coors=None):
        if not features.is_cuda:
            raise lib.Al3dError(f"{type(self).__name__}: device tensors required (no CPU fallback)")
        return self.net(features.device).rows(features.float(), num_voxels)


@READERS.register_module
class VoxelFeatureExtractor(_VFEBase):
    """SECOND's voxel feature extractor (reference voxel_encoder.py:45-108): ``vfe1``, ``vfe2``, ``linear``, ``norm``
    under the reference's parameter names, so its checkpoints load with ``strict=True``.

    ``forward(features [M,T,F], num_voxels [M], coors=None)`` -> ``[M, num_filters[1]]`` from one launch of
    ``al3d_vfe_net_f32`` (csrc/vfe.hip).  As in the reference the padded slots are masked only AFTER ``vfe1``: they enter
    it as ``[0..0, -mean, (0)]`` and take part in its max.  Deviation: a voxel with ``num_voxels == 0`` gives NaN in the
    reference; here it is computed as if every slot were padded (a zero row).  No voxelizer emits one."""

    def __init__(self, num_input_features=4, use_norm=True, num_filters=(32, 128), with_distance=False,
                 voxel_size=(0.2, 0.2, 4), name="VoxelFeatureExtractor"):
        super().__init__()
        self.name = name
        assert len(num_filters) == 2
        nin = num_input_features + 3 + (1 if with_distance else 0)
        self._with_distance = with_distance
        self.vfe1 = VFELayer(nin, num_filters[0], use_norm)
        self.vfe2 = VFELayer(num_filters[0], num_filters[1], use_norm)
        self.linear, self.norm = _vfe_linear_norm(num_filters[1], num_filters[1], use_norm)
        self.out_channels = num_filters[1]
        self._packs = PackCache()

    def _layers(self):
        return [(self.vfe1.linear, self.vfe1.norm), (self.vfe2.linear, self.vfe2.norm), (self.linear, self.norm)]


@READERS.register_module
class VoxelFeatureExtractorV2(_VFEBase):
    """The same reader over a list of VFE layers (reference voxel_encoder.py:111-176): ``vfe_layers.<i>.*``, ``linear``,
    ``norm``.  One or two VFE layers run on the fused kernel; more raise ``NotImplementedError`` (no shipped config has
    them)."""

    def __init__(self, num_input_features=4, use_norm=True, num_filters=(32, 128), with_distance=False,
                 voxel_size=(0.2, 0.2, 4), name="VoxelFeatureExtractor"):
        super().__init__()
        self.name = name
        assert len(num_filters) > 0
        nin = num_input_features + 3 + (1 if with_distance else 0)
        self._with_distance = with_distance
        filters = [nin] + list(num_filters)
        self.vfe_layers = nn.ModuleList([VFELayer(filters[i], filters[i + 1], use_norm) for i in range(len(filters) - 1)])
        self.linear, self.norm = _vfe_linear_norm(filters[-1], filters[-1], use_norm)
        self.out_channels = filters[-1]
        self._packs = PackCache()

    def _layers(self):
        if len(self.vfe_layers) > 2:
            raise NotImplementedError(f"al3d VoxelFeatureExtractorV2: {len(self.vfe_layers)} VFE layers; the fused kernel "
                                      "(al3d_vfe_net_f32) runs one or two")
        return [(v.linear, v.norm) for v in self.vfe_layers] + [(self.linear, self.norm)]


def _slot_mean(features, num_voxels, nfeat, who):
    """Sum of the first ``nfeat`` columns over the T slots / num_voxels (``al3d_vfe_mean_f32``) -> [M, nfeat]."""
    if not features.is_cuda:
        raise lib.Al3dError(f"{who}: device tensors required (no CPU fallback)")
    f = features[:, :, :nfeat].contiguous().float()
    m, t, c = f.shape
    out = torch.empty((m, c), dtype=torch.float32, device=f.device)
    if m:
        num = num_voxels.to(torch.int32).contiguous()
        lib.call("al3d_vfe_mean_f32", _ptr(f), _ptr(num), m, t, c, _ptr(out), _stream())
    return out


@READERS.register_module
class VFEV3_ablation(nn.Module):
    """``[mean_x, mean_y, mean_3, 1/n]`` per voxel (reference voxel_encoder.py:179-194); not a hot path: the slot mean
    from ``al3d_vfe_mean_f32`` and two torch ops on the device."""

    needs_point_slots = True
    mean_reader = False

    def __init__(self, num_input_features=4, norm_cfg=None, name="VFEV3_ablation"):
        super().__init__()
        self.name = name
        self.num_input_features = num_input_features

    def forward(self, features, num_voxels, coors=None):
        mean = _slot_mean(features, num_voxels, 4, "VFEV3_ablation")
        inv = 1.0 / num_voxels.to(torch.float32).view(-1, 1)
        return torch.cat([mean[:, [0, 1, 3]], inv], dim=1).contiguous()


@READERS.register_module
class SimpleVoxel(nn.Module):
    """``[|mean_xy|_2, mean_2..F-1]`` per voxel (reference voxel_encoder.py:214-235); not a hot path: the slot mean from
    ``al3d_vfe_mean_f32`` and a few torch ops on the device."""

    needs_point_slots = True
    mean_reader = False

    def __init__(self, num_input_features=4, norm_cfg=None, name="SimpleVoxel"):
        super().__init__()
        self.num_input_features = num_input_features
        self.name = name

    def forward(self, features, num_voxels, coors=None):
        mean = _slot_mean(features, num_voxels, self.num_input_features, "SimpleVoxel")
        r = torch.sqrt(mean[:, 0:1] * mean[:, 0:1] + mean[:, 1:2] * mean[:, 1:2])
        return torch.cat([r, mean[:, 2:self.num_input_features]], dim=1)
