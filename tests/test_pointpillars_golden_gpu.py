"""GPU suite: the PointPillars kernel and graph against the golden recorded from the reference's own classes
(tools/gen_golden_pointpillars.py -> tests/golden/pointpillars.npz):

  * the pillar kernel (rows and fused canvas) against det3d's and BEVFusion's PillarFeatureNet + PointPillarsScatter;
  * the PointPillars graph -- fused pillars, then this build's RPN loaded through convert_decoder_state_dict -- against
    BEVFusion's SECOND + SECONDFPN with the pointpillars.yaml settings (3 blocks, upsample strides 0.5 / 1 / 2) run on the
    BEVFusion scatter's canvas."""
import os

import numpy as np
import pytest
import torch

import pillars_fp64 as R
from test_bevfusion_second_golden_gpu import seeded_state
from test_pointpillars_golden import golden, golden_geom, golden_layers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(g, neck=True):
    from al3d.models import build_detector
    vs, pr = [float(v) for v in g["voxel_size"]], [float(v) for v in g["pc_range"]]
    m = build_detector(dict(
        type="PointPillars",
        reader=dict(type="PillarFeatureNet", num_input_features=5, num_filters=[64, 64], with_distance=False,
                    voxel_size=vs, pc_range=pr, norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01)),
        backbone=dict(type="PointPillarsScatter", num_input_features=64),
        neck=dict(type="RPN", layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[64, 128, 256],
                  us_layer_strides=[0.5, 1, 2], us_num_filters=[128, 128, 128], num_input_features=64,
                  norm_cfg=dict(eps=1e-3, momentum=0.01)) if neck else None,
        bbox_head=None))
    sd = {k: torch.from_numpy(g["f2_d0." + k]) for k in m.reader.state_dict() if not k.endswith("num_batches_tracked")}
    m.reader.load_state_dict(sd, strict=False)
    return m


def _example(g):
    nx, ny, B = [int(v) for v in g["grid"]]
    return dict(voxels=torch.from_numpy(g["voxels"]).to(DEV), num_points=torch.from_numpy(g["num_points_raw"]).to(DEV),
                coordinates=torch.from_numpy(g["coords"]).to(DEV),
                num_voxels=torch.zeros((B,), dtype=torch.int32, device=DEV),
                shape=np.tile(np.array([[nx, ny, 1]]), (B, 1)), metadata=[{"index": i} for i in range(B)])


@pytest.mark.parametrize("tag", ["f1_d0", "f1_d1", "f2_d0", "f2_d1"])
def test_kernel_matches_the_reference_pillar_nets(tag):
    from al3d.models import build_reader
    g = golden()
    layers = golden_layers(g, tag)
    vs, pr = [float(v) for v in g["voxel_size"]], [float(v) for v in g["pc_range"]]
    r = build_reader(dict(type="PillarFeatureNet", num_input_features=5, num_filters=[64] * len(layers),
                          with_distance=tag.endswith("d1"), voxel_size=vs, pc_range=pr))
    r.load_state_dict({k: torch.from_numpy(g[f"{tag}.{k}"]) for k in r.state_dict()
                       if not k.endswith("num_batches_tracked")}, strict=False)
    r = r.to(DEV).eval()
    ex = _example(g)
    with torch.no_grad():
        got = r(ex["voxels"], ex["num_points"], ex["coordinates"]).cpu().numpy()
    ref, absum = R.pfn_net(g["voxels"], g["num_points_raw"], g["coords"], layers, *golden_geom(g, tag))
    e = float((np.abs(got.astype(np.float64) - ref) / absum).max())
    assert e <= 1.5e-6, f"{tag}: e = {e:.3e} against float64"
    for which in ("out_det3d", "out_bevfusion"):
        want = g[f"{tag}.{which}"]
        e = float((np.abs(got.astype(np.float64) - want) / absum).max())
        assert e <= 3e-6, f"{tag} {which}: e = {e:.3e}"


def test_fused_canvas_matches_the_reference_scatters():
    g = golden()
    m = _model(g, neck=False).to(DEV).eval()
    with torch.no_grad():
        canvas, _ = m.sparse_stage(_example(g))
    got = canvas.cpu().numpy()                                         # [B, ny, nx, C]
    for want in (g["canvas_det3d"].transpose(0, 2, 3, 1), g["canvas_bevfusion"].transpose(0, 3, 2, 1)):
        assert got.shape == want.shape
        assert np.array_equal(got == 0, want == 0)
        assert float(np.abs(got - want).max()) <= 1e-5 * float(np.abs(want).max())


def test_pointpillars_graph_matches_the_reference_decoder():
    from al3d.models.bevfusion_compat import convert_decoder_state_dict
    g = golden()
    sd = {}
    for part, seed, digest in (("backbone", g["decoder_seeds"][0], g["decoder_digest"][0]),
                               ("neck", g["decoder_seeds"][1], g["decoder_digest"][1])):
        part_sd, dig = seeded_state(g[f"keys_{part}"], g[f"shapes_{part}"], seed)
        assert dig == str(digest), part                      # the parameters the reference classes ran with
        sd.update({f"decoder.{part}.{k}": v for k, v in part_sd.items()})
    m = _model(g)
    missing, unexpected = m.neck.load_state_dict(convert_decoder_state_dict(sd, neck_prefix=""), strict=True)
    m = m.to(DEV).eval()
    with torch.no_grad():
        _, middle = m(_example(g), return_loss=False, estimate=True)
        out = middle[-1].nhwc
    ref = torch.from_numpy(g["decoder_out"]).to(DEV).permute(0, 3, 2, 1)   # [B, C, H = x, W = y] -> [B, y, x, C]
    assert out.shape == ref.shape
    err = float((out - ref).abs().max())
    assert err <= 1e-4 * float(ref.abs().max()) + 1e-5, err           # 16 fp32-class convolutions deep
