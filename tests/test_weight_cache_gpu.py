"""Every module that packs convolution weights follows its parameters and keeps one pack per arithmetic
(``al3d.weight_cache.PackCache``): a ``load_state_dict`` after the first forward is served by a fresh pack, and flipping
``AL3D_MATH`` f16x3 -> bf16x6 -> f16x3 (what the ``auto`` sweep does around a tripped batch) packs nothing the third time."""
import os

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _sites(grid, n, seed):
    """n distinct sites of a [1, *grid] grid: coords [n, 4] i32 (b, z, y, x)."""
    flat = torch.randperm(grid[0] * grid[1] * grid[2], generator=torch.Generator().manual_seed(seed))[:n]
    z, y, x = flat // (grid[1] * grid[2]), flat // grid[2] % grid[1], flat % grid[2]
    return torch.stack([torch.zeros_like(z), z, y, x], 1).to(torch.int32).to(DEV)


def _rpn():
    from al3d.models.necks import RPN
    neck = RPN(layer_nums=[1], ds_layer_strides=[1], ds_num_filters=[128], us_layer_strides=[1], us_num_filters=[128],
               num_input_features=256)
    x = _randn(1, 16, 16, 256, seed=1)
    return neck, lambda m: m(x)


def _encoder():
    from al3d.models.backbones import FPNSpMiddleResNetFHD
    coords = _sites((41, 88, 96), 2000, seed=2)
    feats = _randn(2000, 5, seed=3)
    return FPNSpMiddleResNetFHD(num_input_features=5), lambda m: m(feats, coords, 1, [96, 88, 40])[0]


def _spconv():
    from al3d import spconv
    coords = _sites((8, 16, 16), 500, seed=4)
    feats = _randn(500, 16, seed=5)
    net = spconv.SparseSequential(spconv.SubMConv3d(16, 16, 3), nn.BatchNorm1d(16))
    return net, lambda m: m(spconv.SparseConvTensor(feats, coords, [8, 16, 16], 1)).features


def _anchor_head():
    from al3d.models import build_head
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "cbgs_spatial_temporal.py"))
    head = build_head(cfg.model.bbox_head)
    x = _randn(1, 16, 16, head.tasks[0].conv_box.in_channels, seed=6)
    return head, lambda m: m(x)[0]["_fused"]


def _center_head():
    from al3d.models import build_head
    head = build_head(dict(                                             # tests/test_centerhead_gpu.py's HEAD_CFG, graph part
        type="CenterHead", in_channels=32, share_conv_channel=64, norm_bbox=True, transpose_input=True,
        tasks=[["car"], ["truck", "construction_vehicle"], ["pedestrian", "traffic_cone"]],
        common_heads=dict(reg=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2], vel=[2, 2]),
        separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3)))
    x = _randn(1, 16, 16, 32, seed=7)
    return head, lambda m: m(x).fused


def _basic_block():
    from al3d.models.bevfusion_camera_only import BasicBlock
    x = _randn(1, 16, 16, 32, seed=8)
    return BasicBlock(32, 32), lambda m: m(x)


MODULES = dict(rpn=_rpn, encoder=_encoder, spconv=_spconv, anchor_head=_anchor_head, center_head=_center_head,
               basic_block=_basic_block)


def _make(name, seed):
    from al3d import synthetic
    mod, run = MODULES[name]()
    return synthetic.seeded_init_(mod, seed=seed).to(DEV).eval(), run


@pytest.mark.parametrize("name", list(MODULES))
def test_load_state_dict_after_a_forward_is_served_by_a_fresh_pack(name):
    mod, run = _make(name, 11)
    fresh, _ = _make(name, 12)
    with torch.no_grad():
        first = run(mod).clone()
        mod.load_state_dict(fresh.state_dict())
        second = run(mod).clone()
        want = run(fresh)
    assert torch.equal(second, want)
    assert not torch.equal(second, first)


@pytest.mark.parametrize("name", list(MODULES))
def test_flipping_the_arithmetic_and_back_packs_nothing(name, monkeypatch):
    from al3d import detector_ops as D
    packs = []
    for fn in ("dense_pack", "sparse_pack"):
        real = getattr(D, fn)
        monkeypatch.setattr(D, fn, lambda *a, _real=real, _fn=fn, **k: (packs.append(_fn), _real(*a, **k))[1])
    mod, run = _make(name, 13)
    saved = D.MATH
    try:
        with torch.no_grad():
            D.MATH = "f16x3"
            first = run(mod).clone()
            D.MATH = "bf16x6"
            other = run(mod).clone()
            assert packs and torch.isfinite(other).all()
            del packs[:]
            D.MATH = "f16x3"
            third = run(mod)
    finally:
        D.MATH = saved
    assert packs == []
    assert torch.equal(third.view(torch.int32), first.view(torch.int32))
