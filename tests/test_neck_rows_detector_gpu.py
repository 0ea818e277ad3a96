"""GPU suite: the FPNVoxelNet forward with the encoder -> neck hand-over as rows (``AL3D_NECK_IN=rows``,
``detector_ops.BevRows``) against the dense map (``dense``): embeddings and detections identical, in every pipeline mode
of the sweep."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def setup():
    from al3d import synthetic
    from al3d.datasets import DeviceSweepLoader, PoolFrames, generate_task_anchors
    from al3d.models import build_detector
    from al3d.utils import Config
    dev = torch.device(DEV)
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "cbgs_spatial_temporal_feature.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    model = model.to(dev).eval()
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])
    pool = PoolFrames.from_numpy([synthetic.make_point_cloud(77, nsweeps=1), synthetic.make_point_cloud(78, nsweeps=1)], dev)
    # batch_size 1: two batches, so that the pipelined modes hand a batch prepared on the side stream to the main one
    return model, DeviceSweepLoader(pool, cfg.voxel_generator, anchors, batch_size=1, device=dev)


def _count_rows_calls(monkeypatch):
    """Counts the conv2d_nhwc calls that were handed a BevRows."""
    from al3d import detector_ops as D
    seen = []
    conv = D.conv2d_nhwc

    def counting(x, *a, **k):
        if isinstance(x, D.BevRows):
            seen.append(x.shape)
        return conv(x, *a, **k)
    monkeypatch.setattr(D, "conv2d_nhwc", counting)
    return seen


def _sweep(monkeypatch, model, loader, neck_in, pipeline):
    from al3d import detector_ops as D, sweep
    monkeypatch.setattr(D, "NECK_IN", neck_in)
    monkeypatch.setattr(sweep, "PIPELINE", pipeline)
    emb = sweep.sweep_embeddings(model, loader, torch.device(DEV), num_frames=2)
    torch.cuda.synchronize()
    return emb


def _same_words(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_embeddings_identical_rows_and_dense_in_every_pipeline_mode(setup, monkeypatch):
    model, loader = setup
    seen = _count_rows_calls(monkeypatch)
    ref = _sweep(monkeypatch, model, loader, "dense", "ahead")
    assert not seen, "AL3D_NECK_IN=dense must not hand the neck any rows"
    assert ref.shape == (2, 512) and bool(torch.isfinite(ref).all()) and bool((ref != 0).any())
    for pipeline in ("ahead", "split", None):
        before = len(seen)
        emb = _sweep(monkeypatch, model, loader, "rows", pipeline)
        assert len(seen) == before + 2, f"pipeline {pipeline}: the first neck conv of each batch reads the rows"
        assert seen[-1] == (1, 128, 128, 256)
        assert _same_words(emb, ref), f"pipeline {pipeline}"


def test_detections_identical_rows_and_dense(setup, monkeypatch):
    from al3d import detector_ops as D
    model, loader = setup
    example = next(iter(loader))
    seen = _count_rows_calls(monkeypatch)
    out = {}
    for neck_in in ("dense", "rows"):
        monkeypatch.setattr(D, "NECK_IN", neck_in)
        with torch.no_grad():
            preds, middle = model(example, return_loss=False, estimate=True)
        torch.cuda.synchronize()
        out[neck_in] = (preds, middle[-1].nhwc)
    assert len(seen) == 1
    assert _same_words(out["rows"][1], out["dense"][1])
    for a, b in zip(out["rows"][0], out["dense"][0]):
        assert a["box3d_lidar"].shape[1] == 9
        for key in ("box3d_lidar", "scores"):
            assert _same_words(a[key], b[key]), key
        assert torch.equal(a["label_preds"], b["label_preds"])


def test_explicit_stages_and_dense_on_request(setup, monkeypatch):
    """sparse_stage hands out the dense tensor unless asked for rows, also from a book prepared for rows; BevRows.dense()
    is that tensor; the sweep's stream bookkeeping finds the tensors inside a BevRows."""
    from al3d import detector_ops as D, sweep
    model, loader = setup
    monkeypatch.setattr(D, "NECK_IN", "rows")
    example = next(iter(loader))
    with torch.no_grad():
        x_default, _ = model.sparse_stage(example)
        book = model.prepare(example)
        assert "bev_index" in book and "dense" not in book
        x_book, _ = model.sparse_stage(example, book=book)
        x_rows, _ = model.sparse_stage(example, book=book, neck_rows=True)
    assert isinstance(x_default, torch.Tensor) and isinstance(x_book, torch.Tensor) and isinstance(x_rows, D.BevRows)
    assert tuple(x_rows.shape) == tuple(x_default.shape) == (1, 128, 128, 256)
    assert _same_words(x_book, x_default) and _same_words(x_rows.dense(), x_default)
    found = {id(t) for t in sweep._tensors_of((example, (x_rows, [])))}
    assert {id(x_rows.rows), id(x_rows.coords), id(x_rows.index)} <= found
    monkeypatch.setattr(D, "NECK_IN", "dense")
    assert "dense" in model.prepare(example)
