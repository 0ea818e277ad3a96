"""GPU: the registered ``BEVFusion`` detector (camera + lidar) with a ``CenterHead`` under the uncertainty selectors.  The
per-frame entropies of the sweep equal the formula of det3d/selectors/entropy_selector.py:50-86 on ``predict``'s own
``scores``; ``EntropySelector`` ranks by them; ``PPALSelector`` reads the merged int64 ``label_preds`` against the head's
task-grouped ``class_names``.  Seeded weights, synthetic frames (parity unpinned)."""
import json
import os
import pickle
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    from al3d import synthetic
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_camera_lidar_spatial_temporal_feature.py"))
    head = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_lidar_centerhead_entropy.py")).model.bbox_head
    cfg.model.bbox_head = head
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    assert type(model).__name__ == "BEVFusion" and type(model.bbox_head).__name__ == "CenterHead" and model.bbox_head.transpose_input
    synthetic.seeded_init_(model.lidar, seed=0)
    for i, m in enumerate((model.camera_backbone, model.camera_neck, model.vtransform, model.fuser)):
        synthetic.seed_modules_(m, 60 + i)
    synthetic.seeded_init_(model.head, seed=4)
    return cfg, model.to(DEV).eval()


def test_bevfusion_center_head_under_the_entropy_and_ppal_selectors(tmp_path):
    from al3d import sweep as S, synthetic
    from al3d.datasets import CameraLidarSweepLoader, PoolFrames
    from al3d.selectors import build_selector
    cfg, model = _model()
    n = 4
    pool = PoolFrames.from_synthetic(n, DEV, num_base=2, seed=3)
    loader = CameraLidarSweepLoader(pool, cfg.voxel_generator, None, 2, device=DEV, num_image_base=2, seed=1)
    emb, ent = S.sweep_embeddings(model, loader, DEV, n, with_entropy=True)
    assert emb.shape == (n, 512) and ent.shape == (n,)
    nclass = sum(model.bbox_head.num_classes)
    with torch.no_grad():
        ref, counts = [], []
        for ex in loader:
            for o in model(ex, return_loss=False, estimate=True)[0]:
                assert o["box3d_lidar"].shape[1] == 9 and o["label_preds"].dtype == torch.int64
                assert len(o["scores"]) <= 6 * 83 and len(o["scores"]) == len(o["label_preds"]) == len(o["box3d_lidar"])
                if len(o["scores"]):
                    assert 0 <= int(o["label_preds"].min()) and int(o["label_preds"].max()) < nclass
                    assert float(o["scores"].min()) > 0.1
                s = o["scores"].double()
                counts.append(len(s))
                ref.append(float((-s * s.log() - (1 - s) * (1 - s).log()).mean()))      # NaN for a frame without detections
    print("detections per frame", counts, "entropies", ent.cpu().tolist())
    assert sum(c > 0 for c in counts) >= 2, "the seeded model gives too few frames with detections to show anything"
    np.testing.assert_allclose(ent.cpu().numpy(), np.asarray(ref), rtol=5e-6, equal_nan=True)
    infos, _ = synthetic.make_pool(1, seed=0)
    infos = infos[:n]
    ip, bp = str(tmp_path / "infos.pkl"), str(tmp_path / "buffer.json")
    pickle.dump(infos, open(ip, "wb"))
    loader.sampler = list(range(n))
    if bool(torch.isfinite(ent).all()):
        json.dump({"0": []}, open(bp, "w"))
        random.seed(3407)
        sel = build_selector(dict(type="EntropySelector", budget=3, buffer_file=bp, infos_origin=ip, detector=model,
                                  dataloader=loader, pred=True, buffer_path=str(tmp_path / "entropy.pt")))
        sel.select_samples(local_rank=0)
        picked = sel.get_selected_samples()[sel.current_budget]
        order = np.argsort(-ent.cpu().numpy(), kind="stable").tolist()
        assert len(picked) >= 1 and picked == order[:len(picked)]
        assert torch.equal(torch.load(str(tmp_path / "entropy.pt"), weights_only=True), ent.cpu())
    # PPAL: class weights by name over the task groups, labels in the merged label space
    json.dump({"0": [], "1": [1]}, open(bp, "w"))
    cw = str(tmp_path / "cw.json")
    names = [c for g in model.bbox_head.class_names for c in g]
    assert len(names) == nclass == 10
    json.dump({c: 1.0 + 0.1 * i for i, c in enumerate(names)}, open(cw, "w"))
    random.seed(3407)
    sel = build_selector(dict(type="PPALSelector", budget=1, buffer_file=bp, infos_origin=ip, detector=model, dataloader=loader,
                              pred=True, distance_store_file=None, feat_path=str(tmp_path / "pf.pt"), ent_path=str(tmp_path / "pe.pt"),
                              class_weight_file=cw))
    sel.select_samples(local_rank=0)
    picked = sel.get_selected_samples()[sel.current_budget]
    assert 2 <= len(picked) <= n and len(set(picked)) == len(picked) and 1 in picked
