"""CPU suite: the PointPillars registry surface, the example configs, and the float64 restatement (tests/pillars_fp64.py).

The module and parameter names are the reference's (det3d/models/readers/pillar_encoder.py:17-211,
bevfusion/mmdet3d/models/backbones/pillar_encoder.py:47-258), so their checkpoints load by name."""
import os

import numpy as np
import pytest
import torch

import pillars_fp64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ["bevfusion_pointpillars_spatial_temporal_feature.py", "bevfusion_pointpillars_entropy.py"]


@pytest.mark.parametrize("name", CONFIGS)
def test_build_detector_from_example_configs(name):
    from al3d.models import build_detector
    from al3d.models.detectors import PointPillars
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", name))
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    assert isinstance(m, PointPillars)
    assert (m.bbox_head is None) == ("entropy" not in name)
    assert m.prepare({"coordinates": None}) is None
    keys = [k for k in m.state_dict() if k.startswith("reader.")]
    want = [f"reader.pfn_layers.{i}.{k}" for i in range(2) for k in
            ("linear.weight", "norm.weight", "norm.bias", "norm.running_mean", "norm.running_var",
             "norm.num_batches_tracked")]
    assert keys == want
    assert m.reader.pfn_layers[0].linear.weight.shape == (32, 10)      # 5 features + 5 decorations -> 64 // 2
    assert m.reader.pfn_layers[1].linear.weight.shape == (64, 64)
    assert m.reader.pfn_layers[0].norm.eps == 1e-3 and m.reader.pfn_layers[0].norm.momentum == 0.01
    assert not [k for k in m.state_dict() if k.startswith("backbone.")]  # the scatter has no parameters
    if m.bbox_head is not None:
        assert m.bbox_head.in_channels == 384 if hasattr(m.bbox_head, "in_channels") else True


def test_reference_keyword_names():
    """det3d's keywords and BEVFusion's build the same reader; the det3d-style modules build from a bare dict."""
    from al3d.models import build_backbone, build_detector, build_reader
    a = build_reader(dict(type="PillarFeatureNet", num_input_features=5, num_filters=[64, 64], with_distance=True,
                          voxel_size=[0.2, 0.2, 8], pc_range=[-51.2, -51.2, -5, 51.2, 51.2, 3]))
    b = build_reader(dict(type="PillarFeatureNet", in_channels=5, feat_channels=[64, 64], with_distance=True,
                          voxel_size=[0.2, 0.2, 8], point_cloud_range=[-51.2, -51.2, -5, 51.2, 51.2, 3]))
    assert [(k, v.shape) for k, v in a.state_dict().items()] == [(k, v.shape) for k, v in b.state_dict().items()]
    assert a.pfn_layers[0].linear.weight.shape == (32, 11)
    assert abs(a.x_offset - (0.1 - 51.2)) < 1e-12 and abs(b.y_offset - (0.1 - 51.2)) < 1e-12
    s = build_backbone(dict(type="PointPillarsScatter", in_channels=64, output_shape=[512, 512]))
    assert s.nchannels == 64
    m = build_detector(dict(type="PointPillars",
                            reader=dict(type="PillarFeatureNet", num_input_features=4, num_filters=[64]),
                            backbone=dict(type="PointPillarsScatter", num_input_features=64),
                            neck=None, bbox_head=None))
    assert m.reader.pfn_layers[0].linear.weight.shape == (64, 9)


def test_unit_count_outside_the_kernel_is_an_error():
    from al3d import lib
    from al3d.models import build_reader
    r = build_reader(dict(type="PillarFeatureNet", num_input_features=5, num_filters=[24])).eval()
    with pytest.raises(lib.Al3dError, match="multiple of 16"):
        r.net("cpu")
    r = build_reader(dict(type="PillarFeatureNet", num_input_features=5, num_filters=[64, 64, 64])).eval()
    with pytest.raises(lib.Al3dError, match="1 or 2 PFN layers"):
        r.net("cpu")


def _torch_reference(vox, num, coords, mod, xcol, ycol):
    """The reference's forward pass written with torch float64 ops on the module's own parameters."""
    with torch.no_grad():
        return _torch_forward(vox, num, coords, mod, xcol, ycol)


def _torch_forward(vox, num, coords, mod, xcol, ycol):
    f = torch.from_numpy(vox).double()
    n = torch.from_numpy(num).double()
    c = torch.from_numpy(coords).double()
    mean = f[:, :, :3].sum(1, keepdim=True) / n.view(-1, 1, 1)
    fc = torch.stack([f[:, :, 0] - (c[:, xcol:xcol + 1] * mod.vx + mod.x_offset),
                      f[:, :, 1] - (c[:, ycol:ycol + 1] * mod.vy + mod.y_offset)], -1)
    parts = [f, f[:, :, :3] - mean, fc]
    if mod._with_distance:
        parts.append(torch.norm(f[:, :, :3], 2, 2, keepdim=True))
    x = torch.cat(parts, -1)
    mask = (torch.arange(f.shape[1])[None, :] < n[:, None]).double()[..., None]
    x = x * mask
    for i, p in enumerate(mod.pfn_layers):
        y = x @ p.linear.weight.double().t()
        bn = p.norm
        y = (y - bn.running_mean.double()) / torch.sqrt(bn.running_var.double() + bn.eps) * bn.weight.double() + \
            bn.bias.double()
        y = torch.relu(y)
        ymax = y.max(1, keepdim=True)[0]
        if i == len(mod.pfn_layers) - 1:
            return ymax[:, 0].numpy()
        x = torch.cat([y, ymax.repeat(1, f.shape[1], 1)], -1)


@pytest.mark.parametrize("filters", [[64], [64, 64]])
@pytest.mark.parametrize("with_distance", [False, True])
def test_fp64_restatement_matches_module_parameters(filters, with_distance):
    """pillars_fp64 on folded BN == the unfolded float64 forward pass on the module's parameters, in both coordinate
    conventions (this build's / det3d's (b, z, y, x) and BEVFusion's (b, x, y, z))."""
    from al3d.models import build_reader
    from al3d import synthetic
    rng = np.random.default_rng(7)
    mod = build_reader(dict(type="PillarFeatureNet", num_input_features=5, num_filters=filters,
                            with_distance=with_distance, voxel_size=[0.2, 0.2, 8],
                            pc_range=[-51.2, -51.2, -5, 51.2, 51.2, 3]))
    synthetic.seeded_init_(mod, seed=3)
    mod.eval()
    P = 20
    counts = [1, 2, 5, P, P, 7, 3, 19]
    vox, num, coords = R.make_case(rng, len(counts), P, counts=counts)
    coords[0, 2:] = [0, 0]
    coords[1, 2:] = [63, 63]
    layers = []
    for p in mod.pfn_layers:
        bn = p.norm
        s, b = R.fold_bn(bn.weight.detach().numpy(), bn.bias.detach().numpy(), bn.running_mean.numpy(),
                         bn.running_var.numpy(), bn.eps)
        layers.append((p.linear.weight.detach().numpy(), s, b))
    geom = (mod.vx, mod.vy, mod.x_offset, mod.y_offset, with_distance)
    got, absum = R.pfn_net(vox, num, coords, layers, *geom)
    want = _torch_reference(vox, num, coords, mod, 3, 2)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * absum.max())
    bev = coords[:, [0, 3, 2, 1]]                                     # (b, x, y, z)
    got_b, _ = R.pfn_net(vox, num, bev, layers, *geom, xcol=1, ycol=2)
    np.testing.assert_array_equal(got_b, got)
    np.testing.assert_allclose(_torch_reference(vox, num, bev, mod, 1, 2), want, rtol=1e-12, atol=0)
    # the padded slots take part in the max: leaving them out (each pillar cut to its own n slots) changes the result
    cut = np.stack([R.pfn_net(vox[i:i + 1, :n], num[i:i + 1], coords[i:i + 1], layers, *geom)[0][0]
                    for i, n in enumerate(num)])
    padded = num < P
    assert np.array_equal(cut[~padded], got[~padded])
    assert (cut[padded] != got[padded]).any()
