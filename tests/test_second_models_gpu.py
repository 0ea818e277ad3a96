"""GPU suite: det3d's single-stage sparse encoders SpMiddleFHD / SpMiddleResNetFHD and the SECOND model built on them.

Grid input_shape = [96, 88, 40], batch 2 with one empty frame, 2,000 random voxels (tests/second_models_worker.py).
Accuracy against spconv_fp64.encoder_fp64 with the normaliser and the bound of tests/test_spconv_fp64_gpu.py's whole
encoder: 1e-5, argued there as 21 layers at <= 3.5e-7 each (SpMiddleFHD has 14)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import second_models_worker as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev_inputs(name):
    feats, coords = W.make_inputs(W.ENCODERS[name])
    return torch.from_numpy(feats).to(DEV), torch.from_numpy(coords).to(DEV)


def test_resnet_encoder_equals_the_fpn_encoder_bit_for_bit():
    """The same layers and kernels: SpMiddleResNetFHD with a seeded FPNSpMiddleResNetFHD's parameters copied in (by
    position: the FPN encoder splits the same sequence into four stages) gives its dense map."""
    from al3d import synthetic
    from al3d.models import build_backbone
    fpn = build_backbone(dict(type="FPNSpMiddleResNetFHD", num_input_features=5, ds_factor=8, norm_cfg=None))
    synthetic.seeded_init_(fpn, seed=11)
    one = build_backbone(dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8, norm_cfg=None))
    src = list(fpn.state_dict().values())
    one.load_state_dict({k: v.clone() for k, v in zip(one.state_dict(), src)}, strict=True)
    fpn, one = fpn.to(DEV).eval(), one.to(DEV).eval()
    feats, coords = _dev_inputs("SpMiddleResNetFHD")
    with torch.no_grad():
        a, middle = fpn(feats, coords, W.BATCH, W.INPUT_SHAPE)
        b = one(feats, coords, W.BATCH, W.INPUT_SHAPE)
    assert len(middle) == 4 and isinstance(b, torch.Tensor)
    assert tuple(b.shape) == (2, 11, 12, 256) and b.any() and not b[1].any()          # frame 1 is empty
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("name", list(W.ENCODERS))
def test_encoder_vs_fp64_default_arithmetic(name):
    out = W.encoder_error(name)
    print(name, out)
    assert out["zero"] and out["sites"] > 0
    assert out["shape"] == [2, 11, 12, 256 if name == "SpMiddleResNetFHD" else 128]
    assert out["e"] <= 1e-5, f"{name}: e = {out['e']:.3e}"


@pytest.mark.parametrize("math", ["f32", "bf16x6"])
def test_encoders_vs_fp64_other_arithmetics(math):
    """One fresh child process per arithmetic (AL3D_MATH is read when the library's python side is imported)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "second_models_worker.py")],
                       env=dict(os.environ, AL3D_MATH=math), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["math"] == math
    for name in W.ENCODERS:
        assert out[name]["zero"] and out[name]["e"] <= 1e-5, f"{math} {name}: e = {out[name]['e']:.3e}"


@pytest.mark.parametrize("name", list(W.ENCODERS))
def test_book_ahead_and_neck_rows_give_the_same_bits(name):
    from al3d import detector_ops as D
    model = W.build(name).to(DEV)
    feats, coords = _dev_inputs(name)
    with torch.no_grad():
        base = model(feats, coords, W.BATCH, W.INPUT_SHAPE)
        book = model.rulebook_for(coords, W.BATCH, W.INPUT_SHAPE)
        ahead = model(feats, coords, W.BATCH, W.INPUT_SHAPE, book=book)
        assert torch.equal(_bits(ahead), _bits(base))
        rows = model(feats, coords, W.BATCH, W.INPUT_SHAPE, neck_rows=True)
        book = model.rulebook_for(coords, W.BATCH, W.INPUT_SHAPE, neck_rows=True)
        rows_ahead = model(feats, coords, W.BATCH, W.INPUT_SHAPE, book=book, neck_rows=True)
    channels = 128 if name == "SpMiddleResNetFHD" else 64
    applies = D.neck_rows_ok("frag3x3", 2, channels)
    for r in (rows, rows_ahead):
        assert isinstance(r, D.BevRows) == applies
        dense = r.dense() if isinstance(r, D.BevRows) else r
        assert torch.equal(_bits(dense), _bits(base))


# ---------------------------------------------------------------- the SECOND model end to end
@pytest.fixture(scope="module")
def second():
    from al3d import synthetic
    from al3d.datasets import PoolFrames, generate_task_anchors
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "second_vfe_entropy.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    model = model.to(DEV).eval()
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])
    pool = PoolFrames.from_numpy([synthetic.make_point_cloud(s, nsweeps=1) for s in (77, 78)], DEV)
    return cfg, model, anchors, pool


def test_second_model_end_to_end(second):
    """VoxelFeatureExtractor + SpMiddleFHD + RPN + MultiGroupHead on a loader that yields the padded point slots:
    detections and a 512-wide embedding per frame, both bit-identical between two runs."""
    from al3d.datasets import DeviceSweepLoader
    from al3d.models.detectors import NHWCFeature
    from al3d.sweep import sweep_embeddings
    cfg, model, anchors, pool = second
    runs = []
    for _ in range(2):
        loader = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, batch_size=2, device=DEV, with_points=True)
        emb = sweep_embeddings(model, loader, DEV, num_frames=2)
        ex = next(iter(loader))
        assert ex.get("voxels") is not None and ex["voxels"].shape[1:] == (10, 5)
        with torch.no_grad():
            preds = model(ex, return_loss=False)
            x, middle = model.sparse_stage(ex)
            assert middle == [] and tuple(x.shape)[1:] == (128, 128, 128)
            _, middle = model.dense_stage(ex, x, middle, estimate=True)
        assert len(middle) == 1 and isinstance(middle[-1], NHWCFeature)
        runs.append((emb, preds, middle[-1].mean(-1).mean(-1)))
    emb, preds, tap = runs[0]
    assert tuple(emb.shape) == (2, 512) and bool(torch.isfinite(emb).all())
    assert torch.equal(_bits(emb), _bits(tap))
    assert len(preds) == 2 and preds[0]["box3d_lidar"].shape[1] == 9
    assert all(k in preds[0] for k in ("box3d_lidar", "scores", "label_preds"))
    assert torch.equal(_bits(emb), _bits(runs[1][0]))
    for a, b in zip(preds, runs[1][1]):
        for k in ("box3d_lidar", "scores"):
            assert torch.equal(_bits(a[k].float()), _bits(b[k].float()))
        assert torch.equal(a["label_preds"], b["label_preds"])


def test_second_model_needs_the_point_slots(second):
    from al3d.datasets import DeviceSweepLoader
    cfg, model, anchors, pool = second
    loader = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, batch_size=2, device=DEV)
    ex = next(iter(loader))
    assert ex.get("voxels") is None and ex.get("voxel_features") is not None
    with torch.no_grad(), pytest.raises(RuntimeError, match="with_points=True"):
        model(ex, return_loss=False)
