"""CPU suite of the BEV map segmentation head: the float64 yardstick (tests/bev_seg_fp64.py) is pinned to the reference's
own output (tests/golden/bev_seg_head.npz, float32: 1e-5 relative) and to torch's CPU ``F.grid_sample`` + ``nn.Sequential``;
the head builds through the registry with the reference's keys and loads its state dict strictly; the guards raise; the
host tables follow ``torch.arange``'s output size; and the seeded classifier cases of tests/test_bev_seg_gpu.py keep
under 1 % of their pixels within the probability bound of 0.5 (checked here on the yardstick alone)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import bev_seg_fp64 as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bev_seg_head.npz")
_GOLD = {}

# classifier cases of the GPU suite: (C, K, N, H, W); 13 x 21 = 273 pixels: one 256-pixel workgroup and a ragged second one
CLASSIFY_CASES = [(C, K, 2, 13, 21) for C in (32, 256) for K in (1, 6, 16)]


def golden():
    """-> dict(cfg, sd, x, grid, prob, keys), loaded once and left unchanged."""
    if not _GOLD:
        z = np.load(GOLD)
        _GOLD.update(cfg=json.loads(str(z["settings"]))["head"], dtype=json.loads(str(z["settings"]))["dtype"],
                     sd={k[len("sd."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")},
                     x=torch.from_numpy(z["x"]), grid=torch.from_numpy(z["grid"]), prob=torch.from_numpy(z["prob"]),
                     keys=[str(k) for k in z["keys"]])
    return _GOLD


def scopes(cfg):
    return cfg["grid_transform"]["input_scope"], cfg["grid_transform"]["output_scope"]


def classify_case(C, K, N, H, W):
    """Seeded inputs of one classifier case: x [N, H, W, C] channels-last, w [K, C], b [K] (float32)."""
    g = torch.Generator().manual_seed(1000 * C + 10 * K + 1)
    x = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(K, C, generator=g) * (2.0 / C ** 0.5)            # logits of standard deviation 2
    b = torch.randn(K, generator=g)
    return x, w, b


def prob_bound(x, w, b):
    """The issue's bound of the classifier's probabilities without the sigmoid's own error: 0.25 (C + 2) 2^-24
    (sum |w||x| + |b|); 0.25 is the sigmoid's largest slope, C + 2 roundings: the chain's C, the bias, one spare.  NHWC in,
    [N, K, H, W] out."""
    C = x.shape[-1]
    norm = Y.logits64(x.permute(0, 3, 1, 2), w, b, absolute=True)
    return 0.25 * (C + 2) * Y.U * norm


def _rel(got, ref):
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max())


def test_yardstick_matches_the_reference_golden():
    g = golden()
    assert g["dtype"] == "float32"
    i_s, o_s = scopes(g["cfg"])
    grid = Y.resample64(g["x"], i_s, o_s)
    assert tuple(grid.shape) == tuple(g["grid"].shape) and _rel(grid, g["grid"]) < 1e-5
    out = Y.head64(g["x"], g["sd"], i_s, o_s)
    assert tuple(out["prob"].shape) == tuple(g["prob"].shape) == (2, 6, 20, 23) and _rel(out["prob"], g["prob"]) < 1e-5
    # the golden has what the generator asserts: padded rows / columns, exactly zero in the reference too
    mask = Y.padded_mask(i_s, o_s, g["x"].shape[-2:])
    assert bool(mask[0].all()) and bool(mask[:, 0].all()) and not bool(mask[1:, 1:].any())
    assert bool((g["grid"][..., mask] == 0).all()) and bool((grid[..., mask] == 0).all())


def test_yardstick_matches_torch_grid_sample_and_sequential():
    """torch's own CPU path in float64, the reference's forward restated line for line."""
    g = golden()
    i_s, o_s = scopes(g["cfg"])
    x = g["x"].double()
    coords = []
    for (imin, imax, _), (omin, omax, ostep) in zip(i_s, o_s):
        v = torch.arange(omin + ostep / 2, omax, ostep, dtype=torch.float64)
        coords.append((v - imin) / (imax - imin) * 2 - 1)
    u, v = torch.meshgrid(coords, indexing="ij")
    grid = torch.stack([torch.stack([v, u], dim=-1)] * x.shape[0], dim=0)
    ref = F.grid_sample(x, grid, mode="bilinear", align_corners=False)
    assert _rel(Y.resample64(x, i_s, o_s), ref) < 1e-13
    C, K = g["cfg"]["in_channels"], len(g["cfg"]["classes"])
    seq = nn.Sequential(nn.Conv2d(C, C, 3, padding=1, bias=False), nn.BatchNorm2d(C), nn.ReLU(True),
                        nn.Conv2d(C, C, 3, padding=1, bias=False), nn.BatchNorm2d(C), nn.ReLU(True), nn.Conv2d(C, K, 1))
    seq.load_state_dict({k[len("classifier."):]: t for k, t in g["sd"].items()}, strict=True)
    with torch.no_grad():
        z = seq.double().eval()(ref)
    out = Y.head64(g["x"], g["sd"], i_s, o_s)
    assert _rel(out["logits"], z) < 1e-12 and _rel(out["prob"], torch.sigmoid(z)) < 1e-12
    p = torch.sigmoid(z)
    ent = -(p * p.log() + (1 - p) * (1 - p).log())
    assert _rel(out["entropy_sum"], ent.sum((-2, -1))) < 1e-10 and torch.equal(out["area"], (z > 0).sum((-2, -1)))
    # entropy64 at the ends, where the textbook form is 0 * inf
    zz = torch.tensor([-800.0, -40.0, 0.0, 40.0, 800.0], dtype=torch.float64)
    e = Y.entropy64(zz)
    assert bool(torch.isfinite(e).all()) and float(e[0]) == 0.0 and float(e[4]) == 0.0 and abs(float(e[2]) - np.log(2)) < 1e-15


def test_registry_key_set_and_strict_load():
    from al3d.models import HEADS, build_head
    from al3d.models.bev_seg_head import BEVGridTransform, BEVSegmentationHead
    g = golden()
    assert HEADS.get("BEVSegmentationHead") is BEVSegmentationHead
    head = build_head(dict(g["cfg"], type="BEVSegmentationHead"))
    assert sorted(head.state_dict()) == g["keys"]
    head.load_state_dict(g["sd"], strict=True)
    assert isinstance(head.transform, BEVGridTransform) and head.classes == g["cfg"]["classes"] and head.loss == "focal"
    assert tuple(head.classifier[6].weight.shape) == (6, 32, 1, 1) and head.classifier[6].bias is not None
    assert head.classifier[0].bias is None and head.transpose_input is False


def test_guards():
    from al3d import lib
    from al3d.models import build_head
    cfg = golden()["cfg"]
    with pytest.raises(NotImplementedError):
        build_head(dict(cfg, type="BEVSegmentationHead", grid_transform=dict(cfg["grid_transform"], prescale_factor=2)))
    with pytest.raises(lib.Al3dError, match="multiple of 32"):
        build_head(dict(cfg, type="BEVSegmentationHead", in_channels=48))
    head = build_head(dict(cfg, type="BEVSegmentationHead"))
    head.train()
    with pytest.raises(RuntimeError, match="eval"):
        head(torch.zeros(1, 12, 20, 32))
    with pytest.raises(lib.Al3dError):                                # no CPU path: a host tensor is an error, not a detour
        head.eval()(torch.zeros(1, 12, 20, 32))


SCOPES = [((-50.0, 50.0, 0.5), 200), ((-54.0, 54.0, 0.75), 144), ((-7.5, 6.7, 0.7), 20), ((-11.6, 9.0, 0.9), 23),
          ((0.0, 1.0, 0.1), 10), ((0.0, 0.7, 0.1), 7), ((-0.3, 0.3, 0.1), 6), ((-51.2, 51.2, 0.8), 128), ((0.0, 2.1, 0.3), 7),
          ((0.0, 1.15, 0.1), 11)]      # the last: round((omax - omin) / ostep) would say 12


@pytest.mark.parametrize("scope,size", SCOPES)
def test_host_tables_follow_torch_arange(scope, size):
    """The number of outputs is ``len(torch.arange(omin + ostep / 2, omax, ostep))``, whatever (omax - omin) / ostep rounds
    to; indices and weights are the yardstick's, padded taps are (-1, 0)."""
    from al3d import detector_ops as D
    omin, omax, ostep = scope
    n = len(torch.arange(omin + ostep / 2, omax, ostep))
    assert n == size == Y.out_size(*scope)
    for in_scope, in_size in (((-6.0, 6.0, 1.0), 12), ((omin, omax, ostep), 37), ((omin + 0.3, omax + 5.0, 0.4), 9)):
        idx, wgt = D.bev_grid_axis(in_scope, scope, in_size)
        assert idx.shape == (n, 2) and idx.dtype == np.int32 and wgt.shape == (n, 2) and wgt.dtype == np.float32
        i0, w0, w1 = Y.axis64(in_scope, scope, in_size)
        for j, (i, w) in enumerate(((i0, w0), (i0 + 1, w1))):
            inside = ((i >= 0) & (i < in_size)).numpy()
            assert np.array_equal(idx[inside, j], i.numpy()[inside]) and bool((idx[~inside, j] == -1).all())
            assert bool((wgt[~inside, j] == 0).all())
            assert np.array_equal(wgt[inside, j], w.numpy()[inside].astype(np.float32))
        assert bool((wgt >= 0).all()) and bool((wgt <= 1).all())


@pytest.mark.parametrize("case", CLASSIFY_CASES)
def test_seeded_classifier_cases_keep_clear_of_one_half(case):
    """``area`` may differ from the yardstick only at pixels whose float64 probability lies within the probability bound
    of 0.5; the GPU test requires those to be under 1 % of the pixels.  Here: the yardstick alone satisfies that, with the
    bound doubled to leave room for the sigmoid's measured allowance (a few 1e-7 against bounds of 1e-6 and more)."""
    x, w, b = classify_case(*case)
    p = Y.sigmoid64(Y.logits64(x.permute(0, 3, 1, 2), w, b))
    near = (p - 0.5).abs() <= 2.0 * prob_bound(x, w, b) + 1e-6
    assert float(near.double().mean()) < 0.01
    assert 0.2 < float((p > 0.5).double().mean()) < 0.8           # both sides populated


def test_detectors_take_an_optional_map_head():
    """The shipped seg example builds from registered names with the reference's ``heads.map.*`` keys (which the golden
    state dict fits), and both detectors' module trees are unchanged without a map head."""
    from al3d.models import build_detector, build_head
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_camera_seg_spatial_temporal_feature.py"))
    assert cfg.model.bbox_head is None and cfg.selector.type == "SpatialTemporalFeatureSelector"
    det = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    head = det.map_head
    assert det.bbox_head is None and type(head).__name__ == "BEVSegmentationHead" and len(head.classes) == 6
    assert [k for k in det.state_dict() if k.startswith("heads.")] == ["heads.map." + k for k in head.state_dict()]
    assert sorted(head.state_dict()) == golden()["keys"]
    assert head.transform.input_scope[0] == (-51.2, 51.2, 0.8) and head.transform.output_scope[1] == (-50.0, 50.0, 0.5)
    # the registered camera+lidar detector: ``heads.map.*`` beside its own keys, nothing new without a map head
    fcfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_camera_lidar_spatial_temporal_feature.py"))
    plain = build_detector(fcfg.model, train_cfg=None, test_cfg=fcfg.test_cfg)
    map_cfg = dict(cfg.model.map_head, in_channels=512, transpose_input=True)
    fused = build_detector(dict(fcfg.model, map_head=map_cfg), train_cfg=None, test_cfg=fcfg.test_cfg)
    assert not hasattr(plain, "heads") and not any(k.startswith("heads.") for k in plain.state_dict())
    extra = set(fused.state_dict()) - set(plain.state_dict())
    assert extra == {"heads.map." + k for k in build_head(map_cfg).state_dict()} and set(plain.state_dict()) <= set(fused.state_dict())
    assert fused.heads["map"].transpose_input is True
