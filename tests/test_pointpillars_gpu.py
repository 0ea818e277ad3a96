"""GPU suite: the PointPillars pillar kernel (csrc/pillars.hip) against the float64 restatement (tests/pillars_fp64.py),
the canvas it writes, the PointPillars graph, a batch whose canvas crosses 2^31 elements, and the CLI end to end.

Accuracy: e = |got - ref| / absum, absum the abs chain of the winning slot's sums (pillars_fp64.pfn_net), as
tests/test_spconv_fp64_gpu.py measures the sparse convs; bound 1.5e-6."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pillars_fp64 as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = dict(voxel_size=[0.2, 0.2, 8], pc_range=[-51.2, -51.2, -5, 51.2, 51.2, 3])


def _reader(filters, with_distance, seed=3):
    from al3d import synthetic
    from al3d.models import build_reader
    mod = build_reader(dict(type="PillarFeatureNet", num_input_features=5, num_filters=filters,
                            with_distance=with_distance, **GEOM))
    synthetic.seeded_init_(mod, seed=seed)
    return mod.cuda().eval()


def _layers(mod):
    out = []
    for p in mod.pfn_layers:
        bn = p.norm
        s, b = R.fold_bn(bn.weight.detach().cpu().numpy(), bn.bias.detach().cpu().numpy(),
                         bn.running_mean.cpu().numpy(), bn.running_var.cpu().numpy(), bn.eps)
        out.append((p.linear.weight.detach().cpu().numpy(), s, b))
    return out


def _ref(mod, vox, num, coords):
    return R.pfn_net(vox, num, coords, _layers(mod), mod.vx, mod.vy, mod.x_offset, mod.y_offset, mod._with_distance)


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def _err(got, ref, absum):
    return float((np.abs(got.astype(np.float64) - ref) / absum).max()) if ref.size else 0.0


@pytest.mark.parametrize("P", [20, 32])
@pytest.mark.parametrize("filters", [[64], [64, 64]])
@pytest.mark.parametrize("with_distance", [False, True])
@pytest.mark.parametrize("scale", [1e-4, 1.0, 300.0])
def test_kernel_matches_fp64(P, filters, with_distance, scale):
    rng = np.random.default_rng(P * 7 + len(filters) + (11 if with_distance else 0))
    counts = np.concatenate([[1, 2, P, P + 5, P - 1, 3, P + 1], rng.integers(1, P + 1, size=250)])
    vox, num, coords = R.make_case(rng, len(counts), P, counts=counts, scale=scale)
    coords[0, 2:] = [0, 0]                 # grid edges
    coords[1, 2:] = [63, 63]
    coords[2, 2:] = [0, 63]
    mod = _reader(filters, with_distance)
    got = mod(*_dev(vox, num, coords)).cpu().numpy()
    ref, absum = _ref(mod, vox, num, coords)
    assert got.shape == ref.shape
    e = _err(got, ref, absum)
    assert e <= 1.5e-6, f"e = {e:.3e}"


def test_kernel_zero_and_one_pillar():
    mod = _reader([64, 64], False)
    rng = np.random.default_rng(1)
    vox, num, coords = R.make_case(rng, 0, 20)
    out = mod(*_dev(vox, num, coords))
    assert tuple(out.shape) == (0, 64)
    vox, num, coords = R.make_case(rng, 1, 20)
    got = mod(*_dev(vox, num, coords)).cpu().numpy()
    assert got.shape == (1, 64)
    ref, absum = _ref(mod, vox, num, coords)
    assert _err(got, ref, absum) <= 1.5e-6
    from al3d import detector_ops as D
    c = D.pillar_scatter(torch.zeros((0, 64), device="cuda"), torch.zeros((0, 4), dtype=torch.int32, device="cuda"),
                         2, 8, 8)
    assert tuple(c.shape) == (2, 8, 8, 64) and not c.any()


def test_full_frame_60000_pillars():
    """Every pillar of a 512 x 512 frame at the test-time cap, fused into the canvas."""
    rng = np.random.default_rng(5)
    M, P = 60000, 20
    vox, num, coords = R.make_case(rng, M, P, grid=(512, 512), batch=1)
    mod = _reader([64, 64], False)
    net = mod.net(torch.device("cuda"))
    canvas = net.canvas(*_dev(vox, num, coords), 1, 512, 512).cpu().numpy()
    ref, absum = _ref(mod, vox, num, coords)
    got = canvas[coords[:, 0], coords[:, 2], coords[:, 3]]
    assert _err(got, ref, absum) <= 1.5e-6
    hole = np.ones((1, 512, 512), bool)
    hole[coords[:, 0], coords[:, 2], coords[:, 3]] = False
    assert not canvas[hole].any()


def test_canvas_zero_deterministic_split_equals_fused():
    from al3d.models import build_backbone
    rng = np.random.default_rng(9)
    vox, num, coords = R.make_case(rng, 3000, 20, grid=(128, 96), batch=3)
    d = _dev(vox, num, coords)
    mod = _reader([64, 64], True)
    net = mod.net(torch.device("cuda"))
    a = net.canvas(*d, 3, 96, 128)
    b = net.canvas(*d, 3, 96, 128)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    an = a.cpu().numpy()
    hole = np.ones((3, 96, 128), bool)
    hole[coords[:, 0], coords[:, 2], coords[:, 3]] = False
    assert (an[hole].view(np.int32) == 0).all()                     # +0.0 exactly
    rows = mod(*d)
    scatter = build_backbone(dict(type="PointPillarsScatter", num_input_features=64)).cuda()
    split = scatter(rows, d[2], 3, [128, 96, 1])
    assert torch.equal(split.view(torch.int32), a.view(torch.int32))
    assert torch.equal(rows.view(torch.int32), a[d[2][:, 0].long(), d[2][:, 2].long(), d[2][:, 3].long()]
                       .view(torch.int32))


def _small_model(bbox_head=None):
    from al3d import synthetic
    from al3d.models import build_detector
    m = build_detector(dict(
        type="PointPillars",
        reader=dict(type="PillarFeatureNet", num_input_features=5, num_filters=[64, 64], **GEOM),
        backbone=dict(type="PointPillarsScatter", num_input_features=64),
        neck=dict(type="RPN", layer_nums=[1, 1], ds_layer_strides=[2, 2], ds_num_filters=[64, 128],
                  us_layer_strides=[1, 2], us_num_filters=[64, 64], num_input_features=64),
        bbox_head=bbox_head))
    synthetic.seeded_init_(m, seed=0)
    return m.cuda().eval()


def _example(vox, num, coords, B, nx, ny):
    d = _dev(vox, num, coords)
    return dict(voxels=d[0], num_points=d[1], coordinates=d[2],
                num_voxels=torch.zeros((B,), dtype=torch.int32, device="cuda"),
                shape=np.tile(np.array([[nx, ny, 1]]), (B, 1)), metadata=[{"index": i} for i in range(B)])


def test_pointpillars_graph_equals_split_modules():
    """forward(estimate=True): middle[-1] is an NHWCFeature whose GAP equals the neck on the split reader + scatter."""
    from al3d import detector_ops as D
    from al3d.models.detectors import NHWCFeature
    rng = np.random.default_rng(13)
    B, nx, ny = 2, 64, 64
    vox, num, coords = R.make_case(rng, 900, 20, grid=(nx, ny), batch=B)
    m = _small_model()
    ex = _example(vox, num, coords, B, nx, ny)
    with torch.no_grad():
        preds, middle = m(ex, return_loss=False, estimate=True)
        assert len(preds) == B and isinstance(middle[-1], NHWCFeature)
        emb = middle[-1].mean(-1).mean(-1)
        rows = m.reader(ex["voxels"], ex["num_points"], ex["coordinates"])
        canvas = m.backbone(rows, ex["coordinates"], B, [nx, ny, 1])
        y = m.neck(canvas)
        emb2 = m.neck.embedding if m.neck.embedding is not None else D.gap_nhwc(y)
    assert tuple(emb.shape) == (B, 128)
    assert torch.isfinite(emb).all()
    assert torch.equal(emb.view(torch.int32), emb2.view(torch.int32))


def test_batch_canvas_above_2_31_elements():
    """128 frames of a 512 x 512 x 64 canvas (exactly 2^31 floats): the neck runs in frame chunks and the embeddings
    equal those of the same frames run as two batches of 64."""
    from al3d import synthetic
    from al3d.models import build_detector
    m = build_detector(dict(
        type="PointPillars",
        reader=dict(type="PillarFeatureNet", num_input_features=5, num_filters=[64, 64], **GEOM),
        backbone=dict(type="PointPillarsScatter", num_input_features=64),
        neck=dict(type="RPN", layer_nums=[0], ds_layer_strides=[2], ds_num_filters=[64],
                  us_layer_strides=[1], us_num_filters=[64], num_input_features=64),
        bbox_head=None))
    synthetic.seeded_init_(m, seed=1)
    m = m.cuda().eval()
    rng = np.random.default_rng(21)
    B, nx, ny = 128, 512, 512
    vox, num, coords = R.make_case(rng, 128 * 400, 20, grid=(nx, ny), batch=B)
    order = np.argsort(coords[:, 0], kind="stable")
    vox, num, coords = vox[order], num[order], coords[order]
    assert B * ny * nx * 64 >= 1 << 31
    with torch.no_grad():
        _, mid = m(_example(vox, num, coords, B, nx, ny), return_loss=False, estimate=True)
        big = mid[-1].mean(-1).mean(-1).clone()
        del mid
        parts = []
        for lo in (0, 64):
            sel = (coords[:, 0] >= lo) & (coords[:, 0] < lo + 64)
            c = coords[sel].copy()
            c[:, 0] -= lo
            _, mid = m(_example(vox[sel], num[sel], c, 64, nx, ny), return_loss=False, estimate=True)
            parts.append(mid[-1].mean(-1).mean(-1).clone())
            del mid
    small = torch.cat(parts)
    assert big.shape == (B, 64) and torch.isfinite(big).all()
    assert torch.equal(big.view(torch.int32), small.view(torch.int32))


@pytest.mark.parametrize("name,buffer", [
    ("bevfusion_pointpillars_spatial_temporal_feature.py", "bevfusion_pointpillars_stf.json"),
    ("bevfusion_pointpillars_entropy.py", "bevfusion_pointpillars_entropy.json")])
@pytest.mark.parametrize("pipeline", [None, "0"])
def test_cli_pointpillars_configs(tmp_path, name, buffer, pipeline):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "active_select.py"), "--config",
           os.path.join(ROOT, "examples", "active", name), "--budget", "20", "--pred", "--synthetic-scenes", "2",
           "--batch", "8"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    if pipeline is not None:
        env["AL3D_PIPELINE"] = pipeline
    for _ in range(2):                       # bootstrap the empty buffer, then sweep + select
        r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    out = json.load(open(tmp_path / "data" / "buffers" / buffer))
    assert list(out) == ["0", "20"] and len(out["20"]) >= 1 and len(set(out["20"])) == len(out["20"])
