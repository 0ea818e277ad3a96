"""Worker of tests/test_estimator_gpu.py: ``python estimator_sweep_worker.py`` in a fresh process.

``AL3D_PIPELINE`` is read once, when ``al3d.sweep`` is imported, so the sweep's pipelining is a property of the process:
the parent sets the environment, this script sweeps a tiny synthetic pool (three one-sweep clouds, one frame per batch, so
that the pipelined sweep really runs a batch ahead) through the cbgs detector alone and through ``WithEstimator`` and
prints one JSON line with the bit patterns of the per-frame entropies."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    from al3d import sweep as S, synthetic
    from al3d.datasets import DeviceSweepLoader, PoolFrames, generate_task_anchors
    from al3d.models import WithEstimator, build_detector, build_estimator
    from al3d.utils import Config
    dev = torch.device("cuda:0")
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "estimator", "cbgs_partial.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    model = model.to(dev).eval()
    est = build_estimator(cfg.estimator)
    synthetic.seeded_init_(est, seed=5)
    est = est.to(dev).eval()
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])
    pool = PoolFrames.from_numpy([synthetic.make_point_cloud(77 + i, nsweeps=1) for i in range(3)], dev)
    plain = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, batch_size=1, device=dev)
    assert "points" not in next(iter(plain))                # the default batch is unchanged
    kept = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, batch_size=1, device=dev, keep_points=True)
    _, e0 = S.sweep_embeddings(model, plain, dev, num_frames=3, with_entropy=True)
    _, e1 = S.sweep_embeddings(WithEstimator(model, est), kept, dev, num_frames=3, with_entropy=True)
    with torch.no_grad():
        preds, _ = WithEstimator(model, est)(next(iter(kept)), return_loss=False, estimate=True)
        n_boxes = int(preds[0]["scores"].shape[0])
    torch.cuda.synchronize()
    bits = lambda t: t.cpu().numpy().view(np.int32).tolist()     # noqa: E731
    print("RESULT " + json.dumps(dict(pipeline=S.PIPELINE, plain=bits(e0), rescored=bits(e1), boxes_frame0=n_boxes)))


if __name__ == "__main__":
    main()
