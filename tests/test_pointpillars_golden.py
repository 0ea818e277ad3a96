"""CPU suite: the PointPillars float64 restatement (tests/pillars_fp64.py) and the checkpoint converter against the
golden recorded from the reference's own classes (tools/gen_golden_pointpillars.py -> tests/golden/pointpillars.npz):
det3d's and BEVFusion's PillarFeatureNet and PointPillarsScatter, and BEVFusion's SECOND + SECONDFPN with the
pointpillars.yaml settings.  The fixture was recorded behind mmcv / mmdet factory stand-ins (its ``standin`` entry)."""
import os

import numpy as np
import pytest
import torch

import pillars_fp64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "pointpillars.npz")


def golden():
    return np.load(G)


def golden_layers(g, tag):
    layers, i = [], 0
    while f"{tag}.pfn_layers.{i}.linear.weight" in g:
        p = f"{tag}.pfn_layers.{i}."
        s, b = R.fold_bn(g[p + "norm.weight"], g[p + "norm.bias"], g[p + "norm.running_mean"],
                         g[p + "norm.running_var"], 1e-3)
        layers.append((g[p + "linear.weight"], s, b))
        i += 1
    return layers


def golden_geom(g, tag):
    vs, pr = g["voxel_size"], g["pc_range"]
    return (float(vs[0]), float(vs[1]), float(vs[0]) / 2 + float(pr[0]), float(vs[1]) / 2 + float(pr[1]),
            tag.endswith("d1"))


def test_golden_fixture_shape():
    g = golden()
    assert "factory stand-ins" in str(g["standin"])
    assert os.path.getsize(G) < 1 << 20
    raw, P = g["num_points_raw"], g["voxels"].shape[1]
    assert (raw == 1).any() and (raw == P).any() and (raw > P).any() and ((raw > 1) & (raw < P)).any()
    nx, ny, B = g["grid"]
    c = g["coords"]
    assert set(np.unique(c[:, 0])) == {0, 2}                       # frame 1 is empty
    assert (c[:, 3] == 0).any() and (c[:, 3] == nx - 1).any() and (c[:, 2] == ny - 1).any()
    assert list(g["cases"]) == ["f1_d0", "f1_d1", "f2_d0", "f2_d1"]


@pytest.mark.parametrize("tag", ["f1_d0", "f1_d1", "f2_d0", "f2_d1"])
def test_fp64_restatement_matches_reference_pillar_nets(tag):
    """Both reference PillarFeatureNets (det3d on (b, z, y, x), BEVFusion on (b, x, y, z)), [64] / [64, 64], with_distance
    off / on; counts above P are clipped like the voxelizer does."""
    g = golden()
    layers, geom = golden_layers(g, tag), golden_geom(g, tag)
    vox, raw, c = g["voxels"], g["num_points_raw"], g["coords"]
    ref, absum = R.pfn_net(vox, raw, c, layers, *geom)
    bev, _ = R.pfn_net(vox, raw, c[:, [0, 3, 2, 1]], layers, *geom, xcol=1, ycol=2)
    for want, got in ((g[f"{tag}.out_det3d"], ref), (g[f"{tag}.out_bevfusion"], bev)):
        assert want.shape == got.shape
        e = float((np.abs(want.astype(np.float64) - got) / absum).max())
        assert e <= 2e-6, f"{tag}: e = {e:.3e}"                      # the reference ran in float32


def test_scatter_restatement_matches_reference_scatters():
    g = golden()
    nx, ny, B = [int(v) for v in g["grid"]]
    c = g["coords"]
    det = R.scatter_nhwc(g["f2_d0.out_det3d"], c, B, ny, nx)
    assert np.array_equal(det, g["canvas_det3d"].transpose(0, 2, 3, 1))          # [B, C, ny, nx] there
    bev = R.scatter_nhwc(g["f2_d0.out_bevfusion"], c, B, ny, nx)
    assert np.array_equal(bev, g["canvas_bevfusion"].transpose(0, 3, 2, 1))      # [B, C, nx, ny] there


def bevfusion_state_dict(g, head=None):
    """A BEVFusion pointpillars.yaml-shaped state dict: the reference PFN keys with the golden's f2_d0 weights, the
    reference SECOND / SECONDFPN keys and shapes, and (optionally) a head under heads.object."""
    sd = {}
    for k in g["pfn_keys_bevfusion"]:
        k = str(k)
        sd["encoders.lidar.backbone.pts_voxel_encoder." + k] = \
            torch.zeros((), dtype=torch.int64) if k.endswith("num_batches_tracked") else torch.from_numpy(g["f2_d0." + k])
    for part in ("backbone", "neck"):
        for k, shp in zip(g[f"keys_{part}"], g[f"shapes_{part}"]):
            sd[f"decoder.{part}.{k}"] = torch.randn(eval(str(shp)))
    for k, v in (head or {}).items():
        sd["heads.object." + k] = v.clone()
    return sd


@pytest.mark.parametrize("name", ["bevfusion_pointpillars_spatial_temporal_feature.py", "bevfusion_pointpillars_entropy.py"])
def test_converter_maps_a_bevfusion_checkpoint_with_nothing_missing(name):
    from al3d.models import build_detector
    from al3d.models.bevfusion_compat import convert_pointpillars_state_dict
    from al3d.utils import Config
    g = golden()
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", name))
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    head = m.bbox_head.state_dict() if m.bbox_head is not None else None
    sd = bevfusion_state_dict(g, head)
    conv = convert_pointpillars_state_dict(sd)
    missing, unexpected = m.load_state_dict(conv, strict=True)
    assert not missing and not unexpected
    w = sd["decoder.backbone.blocks.0.0.weight"]
    assert torch.equal(m.neck.blocks[0][1].weight, w.transpose(2, 3))          # 3x3 kernels: H = y here
    up = sd["decoder.neck.deblocks.0.0.weight"]                                    # the 0.5-stride 2x2/s2 conv
    assert up.shape[-1] == 2 and torch.equal(m.neck.deblocks[0][0].weight, up.transpose(2, 3))
    assert torch.equal(m.reader.pfn_layers[1].linear.weight, sd["encoders.lidar.backbone.pts_voxel_encoder."
                                                                "pfn_layers.1.linear.weight"])
    with pytest.raises(KeyError):
        convert_pointpillars_state_dict({k: v for k, v in sd.items() if "pfn_layers.0.norm.running_var" not in k})
