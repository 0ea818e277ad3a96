"""GPU suite of what is built on the box IoU / NMS ops: the Estimator-target pre-pass (``sweep_iou_targets``), alone and under
two gloo ranks, and ``TransFusionHead(test_cfg.nms_type="rotate")`` on planted proposals against the float64 greedy loop
of tests/box_iou_cases.py."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import box_iou_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---------------------------------------------------------------- the pre-pass
def test_sweep_iou_targets_equals_box_iou_best_on_the_collected_buffers():
    """A 4-frame synthetic pool through the seeded detector in two batches: the rows ``sweep_iou_targets`` returns are, frame
    by frame, ``box_iou_best`` on that batch's raw NMS buffers, compacted to the valid slots in order.  The ground truth is
    the sweep's own detections, moved a little, so the targets are real IoUs and not all 1."""
    from al3d import selector_ops as ops
    from al3d.datasets import DeviceSweepLoader, PoolFrames, generate_task_anchors
    from al3d.models import build_detector
    from al3d.selectors import prepass as P
    from al3d.utils import Config
    from al3d import synthetic
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "cbgs_cald.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    model = model.to(DEV).eval()
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])
    pool = PoolFrames.from_synthetic(4, DEV, num_base=4, seed=3, nsweeps=1)
    loader = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, 2, device=DEV)
    dets = P.sweep_detections(model, loader, DEV, 4)
    assert len(dets.boxes) >= 8 and dets.boxes.shape[1] == 9
    rng = np.random.default_rng(2)
    gt = dets.boxes.copy()
    gt[:, :2] += rng.uniform(-0.4, 0.4, (len(gt), 2)).astype(np.float32)
    gt[:, 8] += rng.uniform(-0.2, 0.2, len(gt)).astype(np.float32)
    keep = rng.uniform(size=len(gt)) < 0.8                                    # some detections have no box of their own
    off = np.concatenate([[0], np.cumsum([keep[dets.off[i]:dets.off[i + 1]].sum() for i in range(4)])])
    refs = P.FrameRefs(gt[keep], dets.labels[keep], dets.scores[keep], off)
    for same_class in (False, True):
        got = P.sweep_iou_targets(model, loader, DEV, refs, same_class=same_class)
        want = {k: [] for k in ("best_iou", "best_ref", "scores", "labels")}
        counts_all = []
        for ids, preds in P._batches(model, loader, DEV):
            boxes, scores, labels, counts = P._raw_of(preds)
            rb, rl, _, roff = refs.batch(ids, DEV)
            iou, ref = ops.box_iou_best(boxes, labels, counts, rb, rl, roff, metric="iou3d", ref_rot_col=8, same_class=same_class)
            for b, i in enumerate(ids):
                for t in range(boxes.shape[1]):
                    k = min(max(int(counts[b, t]), 0), boxes.shape[2])
                    r = ref[b, t, :k].long().cpu().numpy()
                    want["best_ref"].append(np.where(r >= 0, r - int(roff[b]) + refs.off[i], -1))
                    want["best_iou"].append(iou[b, t, :k].cpu().numpy())
                    want["scores"].append(scores[b, t, :k].cpu().numpy())
                    want["labels"].append(labels[b, t, :k].cpu().numpy())
                counts_all.append(int(counts[b].clamp(0, boxes.shape[2]).sum()))
        assert got["off"].tolist() == np.concatenate([[0], np.cumsum(counts_all)]).tolist()
        for k, v in want.items():
            v = np.concatenate(v)
            assert got[k].shape == v.shape and np.array_equal(got[k], v.astype(got[k].dtype)), k
        assert got["best_iou"].dtype == np.float32 and got["best_ref"].dtype == np.int64
        hit = got["best_ref"] >= 0
        assert hit.sum() >= 8 and 0.3 < got["best_iou"][hit].max() < 1.0
        if same_class:
            assert (refs.labels[got["best_ref"][hit]] == got["labels"][hit]).all()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_return_the_rows_in_dataset_order(tmp_path):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "iou_targets_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    assert [x["rows"] for x in recs] == [3, 2]
    for x in recs:
        assert x["world"] == 2 and x["ok_0"] and x["ok_1"], x
        assert x["matched_0"] == 11 and 0 < x["matched_1"] <= 11, x          # frame 2 has detections and no ground truth


# ---------------------------------------------------------------- TransFusionHead, nms_type = "rotate"
def _planted_head_outputs():
    """Eight proposals of one sample as the decoder would emit them: two pedestrians that overlap (IoU 0.54), two that barely
    do (0.05), two overlapping cars (no NMS for their task: radius -1), two overlapping cones (IoU 0.4 against 0.175)."""
    rows = [  # class, x, y, w, l, r, score
        (8, -40.0, -30.0, 0.67, 0.73, 0.0, 0.9), (8, -39.8, -30.0, 0.67, 0.73, 0.0, 0.8),
        (8, -50.0, -20.0, 0.67, 0.73, 0.3, 0.7), (8, -49.4, -20.0, 0.67, 0.73, 0.3, 0.75),
        (0, -30.0, -35.0, 1.97, 4.63, 1.0, 0.6), (0, -29.7, -35.2, 1.97, 4.63, 1.1, 0.65),
        (9, -45.0, -12.0, 0.41, 0.41, 0.5, 0.5), (9, -44.85, -12.05, 0.41, 0.41, 0.2, 0.55)]
    return np.asarray(rows, np.float64)


def test_transfusion_rotate_nms_keeps_what_the_float64_loop_keeps():
    from test_transfusion_gpu import _cfg, _seed_
    from al3d.models.transfusion_head import TransFusionHead
    rows = _planted_head_outputs()
    P = len(rows)
    head = _seed_(TransFusionHead(**_cfg(num_proposals=P, test_cfg=dict(nms_type="rotate", pre_maxsize=1000, post_maxsize=83))), 3).to(DEV)
    bc = head.bbox_coder
    cls = rows[:, 0].astype(np.int64)
    logit = lambda p: np.log(p / (1 - p))                                     # noqa: E731
    heat = np.full((1, 10, P), -20.0)
    heat[0, cls, np.arange(P)] = logit(rows[:, 6])
    center = np.stack([(rows[:, 1] - bc["pc_range"][0]) / (bc["out_size_factor"] * bc["voxel_size"][0]),
                       (rows[:, 2] - bc["pc_range"][1]) / (bc["out_size_factor"] * bc["voxel_size"][1])])[None]
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV)         # noqa: E731
    preds = dict(heatmap=t(heat), center=t(center), height=t(np.full((1, 1, P), 0.5)),
                 dim=t(np.log(np.stack([rows[:, 3], rows[:, 4], np.full(P, 1.7)]))[None]),
                 rot=t(np.stack([np.sin(rows[:, 5]), np.cos(rows[:, 5])])[None]), vel=t(np.zeros((1, 2, P))),
                 query_heatmap_score=t(np.ones((1, 10, P))))
    head.query_labels = torch.as_tensor(cls[None], device=DEV)
    head.test_cfg["nms_type"] = None
    plain = head.get_bboxes([preds])[0]
    assert plain["bboxes"].shape == (P, 9) and plain["labels"].cpu().tolist() == cls.tolist()
    head.test_cfg["nms_type"] = "rotate"
    got = head.get_bboxes([preds])[0]
    # the float64 loop per task on the boxes the head decoded (float32 numbers, taken as they are)
    b = plain["bboxes"].cpu().numpy().astype(np.float64)
    s = plain["scores"].cpu().numpy()
    x32, rows64 = C.xyxyr_rows(np.stack([b[:, 0], b[:, 1], 0 * b[:, 0], b[:, 3], b[:, 4], 0 * b[:, 0], b[:, 6]], 1))
    iou = C.metric_matrix(C.inter_matrix64(rows64, rows64, "det3d"), rows64, rows64, "iou", "_bev")
    keep = np.zeros(P, bool)
    decided = []
    for classes, radius in (((0, 1, 2, 3, 4, 5, 6, 7), -1), ((8,), 0.175), ((9,), 0.175)):
        idx = np.nonzero(np.isin(cls, classes))[0]
        if radius <= 0:
            keep[idx] = True
            continue
        pairs = {(i, j): iou[idx[i], idx[j]] for i in range(len(idx)) for j in range(i + 1, len(idx))}
        decided += [abs(v - radius) for v in pairs.values()]
        keep[idx[C.nms64(C._SparseIou(pairs), s[idx], radius, 1000, 83)]] = True
    assert min(decided) > C.BAND_DECIDE
    assert keep.tolist() == [True, False, True, True, True, True, False, True]
    assert got["labels"].cpu().tolist() == cls[keep].tolist()
    assert torch.equal(got["bboxes"], plain["bboxes"][torch.as_tensor(keep, device=DEV)])
    assert torch.equal(got["scores"], plain["scores"][torch.as_tensor(keep, device=DEV)])
    assert got["bboxes"].is_cuda
