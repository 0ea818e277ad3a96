"""Dev tool (needs the reference tree; not run by the tests).  Golden vectors of the box-wise IoU estimator:
tests/golden/estimator.npz, arrays only.

The reference's OWN ``Estimator`` (det3d/models/detectors/estimator.py:22-274) is imported through oracle/ref_import.py and
its ``extract_points_feature_gpu`` and ``estimate`` run on CPU, frame by frame (a frame in which no box survives makes its
``torch.stack([])`` raise: that is asserted, and such frames are recorded as empty).  Stand-ins registered here, none with
algorithmic content beyond the first: ``torch_scatter.scatter_max`` = ``Tensor.scatter_reduce(0, index, src, "amax",
include_self=False)`` (argmax not returned: the reference takes ``[0]``); empty leaves for ``open3d``,
``det3d.ops.iou3d_nms``, ``det3d.ops.pointnet2``, ``det3d.core.sampler.preprocess`` and
``det3d.models.detectors.single_stage`` (its ``SingleStageDetector`` = ``nn.Module``; only the out-of-scope DETECTORS
variant derives from it).

The float64 restatement tests/estimator_numpy.py is evaluated on the same inputs and asserted against the reference:
membership counts and survivors exactly, features and IoUs to f32 rounding.  ``ref_f32_gap`` = max |reference f32 IoU -
float64 IoU| is stored; the tests' tolerance is 4 x that.

Fixture condition, enforced: before the reference runs, every point closer than 1e-3 m to an edge of any doubled
footprint of its frame, or with ||pz - z| - h/2| < 1e-3 m for any box of its frame, is dropped (membership is a strict
inequality on f32 products: such a point may legitimately flip); more than 5 % dropped refuses to write.

  python tools/gen_golden_estimator.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import as RI  # noqa: E402
import estimator_numpy as EN  # noqa: E402

B, NT, POST, D, F = 4, 2, 8, 9, 5
TASKS = [dict(num_class=4, class_names=["car", "truck", "bus", "trailer"]),
         dict(num_class=6, class_names=["barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone", "cv"])]
NC = 10
MARGIN = 1e-3
POINTS = (1300, 70, 0, 1300)
COUNTS = np.array([[8, 8], [1, 8], [8, 1], [0, 0]], dtype=np.int32)


def scatter_max(src, index, dim=0):
    out = src.new_zeros((int(index.max()) + 1,) + tuple(src.shape[1:]))
    idx = index.view(-1, *([1] * (src.dim() - 1))).expand_as(src)
    return out.scatter_reduce(dim, idx, src, "amax", include_self=False), None


def import_reference_estimator():
    RI.install_standins()
    ref = RI.REFERENCE_ROOT
    RI._mod("torch_scatter", scatter_max=scatter_max)
    RI._mod("open3d")
    for pkg in ("det3d.ops", "det3d.core", "det3d.core.bbox", "det3d.core.sampler", "det3d.models", "det3d.models.detectors"):
        if pkg not in sys.modules:
            RI._pkg(pkg, os.path.join(ref, *pkg.split(".")))
    RI._mod("det3d.ops.iou3d_nms", boxes_iou3d_gpu=None)
    RI._mod("det3d.ops.pointnet2", pointnet2_utils=None)
    RI._mod("det3d.core.sampler.preprocess")
    RI._mod("det3d.models.detectors.single_stage", SingleStageDetector=nn.Module)
    RI.import_box_np_ops()
    RI.import_box_torch_ops()
    # det3d.core.bbox is a seeded package object: the names estimator.py takes from it are its sub-modules
    core_bbox = sys.modules["det3d.core.bbox"]
    core_bbox.geometry = importlib.import_module("det3d.core.bbox.geometry")
    core_bbox.box_torch_ops = importlib.import_module("det3d.core.bbox.box_torch_ops")
    sys.modules["det3d.core.sampler"].preprocess = sys.modules["det3d.core.sampler.preprocess"]
    return importlib.import_module("det3d.models.detectors.estimator")


def poly_to_world(box, u, v):
    """World xy of the footprint-local position (u, v) (the polygon's sense of rotation)."""
    c, s = np.cos(float(box[6])), np.sin(float(box[6]))
    return u * c + v * s + float(box[0]), -u * s + v * c + float(box[1])


def feat_to_world(box, a, b):
    """World xy of the position whose FEATURE-frame offset is (a, b) (the other sense)."""
    c, s = np.cos(float(box[6])), np.sin(float(box[6]))
    return a * c - b * s + float(box[0]), a * s + b * c + float(box[1])


def make_inputs(rng):
    boxes = np.zeros((B, NT, POST, D), dtype=np.float32)
    labels = np.zeros((B, NT, POST), dtype=np.int32)
    scores = rng.uniform(0.05, 0.95, size=(B, NT, POST)).astype(np.float32)
    # every slot (valid or not) starts as a random box on a 25 m grid cell of its own
    cells = [(gx, gy) for gx in (-37.5, -12.5, 12.5, 37.5) for gy in (-37.5, -12.5, 12.5, 37.5)]
    for b in range(B):
        order = rng.permutation(len(cells))
        for t in range(NT):
            for i in range(POST):
                gx, gy = cells[order[t * POST + i]]
                w, l, h = rng.uniform(0.6, 2.5), rng.uniform(0.8, 4.5), rng.uniform(1.0, 3.0)
                # column 6 is what the reference reads as the angle (box[:, :7][:, -1]); both signs, beyond +-pi
                ang = rng.uniform(-7.0, 7.0)
                boxes[b, t, i] = [gx + rng.uniform(-2, 2), gy + rng.uniform(-2, 2), rng.uniform(-1, 1), w, l, h,
                                  ang, rng.normal(), rng.uniform(-3, 3)]
                labels[b, t, i] = rng.integers(0, 4) if t == 0 else 4 + rng.integers(0, 6)
    frames = []
    # ---- frame 0: the rich one
    bx = boxes[0]
    pts = []

    def add(box, uv, z):
        x, y = poly_to_world(box, uv[:, 0], uv[:, 1])
        pts.append(np.stack([x, y, z], 1))

    def cloud(box, n, spread=1.3, zspread=1.0):
        w, l, h = float(box[3]), float(box[4]), float(box[5])
        uv = rng.uniform(-spread, spread, size=(n, 2)) * [w, l]
        add(box, uv, float(box[2]) + rng.uniform(-zspread, zspread, size=n) * h)

    # two overlapping boxes sharing points: (0,0,1) sits 1 m from (0,0,0)
    bx[0, 1, :3] = bx[0, 0, :3] + np.float32([0.8, 0.6, 0.1])
    cloud(bx[0, 0], 90)
    cloud(bx[0, 1], 60)
    # a box with exactly one point
    add(bx[0, 2], np.array([[0.3 * bx[0, 2, 3], -0.4 * bx[0, 2, 4]]]), np.array([bx[0, 2, 2] + 0.1]))
    # points only in the expanded ring: beyond the box's own half width in the FEATURE frame (negative centerness), kept
    # where the doubled footprint (the polygon's sense of rotation) still holds them
    w, l = float(bx[0, 3, 3]), float(bx[0, 3, 4])
    a, b_ = rng.choice([-1, 1], 600) * rng.uniform(0.55, 1.0, 600) * w, rng.uniform(-1.0, 1.0, 600) * l
    x, y = feat_to_world(bx[0, 3], a, b_)
    cand = np.stack([x, y, bx[0, 3, 2] + rng.uniform(-0.4, 0.4, 600) * bx[0, 3, 5]], 1)
    cand = cand[EN.inside(cand, bx[0, 3])][:40]
    pts.append(cand)
    # inside the BEV footprint, outside the height: the box is dropped
    uv = rng.uniform(-0.9, 0.9, size=(30, 2)) * [bx[0, 4, 3], bx[0, 4, 4]]
    add(bx[0, 4], uv, bx[0, 4, 2] + rng.choice([-1, 1], 30) * rng.uniform(0.55, 2.0, 30) * bx[0, 4, 5])
    # the rotation quirk, w = 1, l = 3, angle 0.8: feature-frame offset (1.1 w, 0) is inside only because the polygon
    # rotates the other way, (0, 0.9 l) is outside for the same reason
    for i, (a, b_) in ((5, (1.1, 0.0)), (6, (0.0, 2.7))):
        bx[0, i, 3:7] = [1.0, 3.0, 2.0, 0.8]
        x, y = feat_to_world(bx[0, i], a, b_)
        pts.append(np.array([[x, y, float(bx[0, i, 2])]]))
    # (0,0,7) keeps no point at all; the second task: general clouds, one box without points
    for i in range(POST):
        if i != 3:
            cloud(bx[1, i], int(rng.integers(20, 90)))
    n_fg = sum(len(p) for p in pts)
    # background: above every box (inside footprints, outside heights) and far ground clutter between the cells
    bg = np.stack([rng.uniform(-50, 50, POINTS[0] - n_fg), rng.uniform(-50, 50, POINTS[0] - n_fg),
                   rng.uniform(6.0, 9.0, POINTS[0] - n_fg)], 1)
    frames.append(np.concatenate(pts + [bg]))
    # ---- frame 1: 70 points, every box far from them (no box holds a point)
    boxes[1, :, :, 0] = np.abs(boxes[1, :, :, 0]) * 0.3 + 30.0
    frames.append(np.stack([rng.uniform(-45, 5, POINTS[1]), rng.uniform(-45, 45, POINTS[1]), rng.uniform(-2, 2, POINTS[1])], 1))
    # ---- frame 2: no points at all; frame 3: points in and around boxes whose slots are NOT valid (counts 0)
    frames.append(np.zeros((0, 3)))
    pts = []
    for t in range(NT):
        for i in range(POST):
            w, l, h = boxes[3, t, i, 3:6]
            uv = rng.uniform(-0.9, 0.9, size=(40, 2)) * [w, l]
            x, y = poly_to_world(boxes[3, t, i], uv[:, 0], uv[:, 1])
            pts.append(np.stack([x, y, boxes[3, t, i, 2] + rng.uniform(-0.4, 0.4, 40) * h], 1))
    n_fg = sum(len(p) for p in pts)
    pts.append(np.stack([rng.uniform(-50, 50, POINTS[3] - n_fg), rng.uniform(-50, 50, POINTS[3] - n_fg),
                         rng.uniform(-3, 3, POINTS[3] - n_fg)], 1))
    frames.append(np.concatenate(pts))
    out = []
    for f in frames:                                        # shuffled, with two extra columns (intensity, time)
        f = f[rng.permutation(len(f))]
        out.append(np.concatenate([f, rng.uniform(0, 1, size=(len(f), F - 3))], 1).astype(np.float32))
    return boxes, scores, labels, out


def enforce_margin(boxes, frames):
    """Drop the points within MARGIN of a membership boundary of any VALID box of their frame; -> (frames, share)."""
    kept, total, dropped = [], 0, 0
    for b, f in enumerate(frames):
        ok = np.ones(len(f), dtype=bool)
        p = f.astype(np.float64)
        for t in range(NT):
            for i in range(int(COUNTS[b, t])):
                box = boxes[b, t, i]
                if len(f):
                    ok &= EN.edge_distance(p[:, :2], EN.footprint(box)) >= MARGIN
                    ok &= np.abs(np.abs(p[:, 2] - float(box[2])) - float(box[5]) / 2) >= MARGIN
        total += len(f)
        dropped += int((~ok).sum())
        kept.append(f[ok])
    return kept, dropped / max(total, 1)


def seeded_estimator(cls):
    torch.manual_seed(20)
    m = cls(tasks=TASKS, dim_feat=224)
    g = torch.Generator().manual_seed(21)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm1d):                 # non-identity statistics
            mod.weight.data = torch.rand(mod.num_features, generator=g) + 0.5
            mod.bias.data = torch.randn(mod.num_features, generator=g) * 0.1
            mod.running_mean.data = torch.randn(mod.num_features, generator=g) * 0.2
            mod.running_var.data = torch.rand(mod.num_features, generator=g) * 1.5 + 0.5
    return m.eval()


def main():
    rng = np.random.default_rng(2024)
    ref_mod = import_reference_estimator()
    boxes, scores, labels, frames = make_inputs(rng)
    frames, share = enforce_margin(boxes, frames)
    assert share <= 0.05, f"{share:.3%} of the points lie within {MARGIN} m of a boundary: refusing to write"
    # the point counts the shapes ask for, after the drop: pad with far-away points (no box within 100 m of them)
    for b in range(B):
        lack = POINTS[b] - len(frames[b])
        assert lack >= 0
        if lack and POINTS[b]:
            far = np.concatenate([rng.uniform(200, 300, size=(lack, 2)), rng.uniform(-1, 1, size=(lack, 1)),
                                  rng.uniform(0, 1, size=(lack, F - 3))], 1).astype(np.float32)
            frames[b] = np.concatenate([frames[b], far])[rng.permutation(POINTS[b])]
    assert tuple(len(f) for f in frames) == POINTS
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    points = np.concatenate(frames).astype(np.float32)

    # the module's name `Estimator` is rebound by the DETECTORS variant further down (:343); the registry holds the one meant
    est = seeded_estimator(ref_mod.ESTIMATORS.get("Estimator"))
    state = {k: v.detach().numpy().copy() for k, v in est.state_dict().items()}
    y = EN.run(boxes, labels, COUNTS, points, offsets, state, NC)

    ref_npts = np.zeros((B, NT, POST), dtype=np.int64)
    ref_iou = np.full((B, NT, POST), np.nan, dtype=np.float32)
    ref_pooled = np.zeros((B, NT, POST, 128), dtype=np.float32)
    ref_survivors = []
    feat_pairs, feat_ref = [], []
    with torch.no_grad():
        for b in range(B):
            slots = [(t, i) for t in range(NT) for i in range(int(COUNTS[b, t]))]
            bb = torch.from_numpy(np.stack([boxes[b, t, i] for t, i in slots])) if slots else torch.zeros((0, D))
            pred = dict(box3d_lidar=bb, scores=torch.from_numpy(np.array([scores[b, t, i] for t, i in slots], np.float32)),
                        label_preds=torch.from_numpy(np.array([labels[b, t, i] for t, i in slots], np.int64)),
                        metadata=dict(token=f"f{b}"))
            pts = torch.from_numpy(np.concatenate([np.zeros((len(frames[b]), 1), np.float32), frames[b]], 1))
            example = dict(preds=[pred], points=pts, middle=None)
            try:
                feats, inst, rb, sc, lb = est.extract_points_feature_gpu(example)
            except RuntimeError as e:                       # torch.stack([]) of a frame without survivors
                assert "non-empty" in str(e) or "empty" in str(e), e
                assert int(y["counts"][b].sum()) == 0, "the reference raised on a frame the restatement keeps boxes in"
                ref_survivors += [[] for _ in range(NT)]
                continue
            kept_boxes = example["preds"][0]["box3d_lidar"].numpy()
            kept = []
            for row in kept_boxes:                          # the surviving rows, in order, back to their slots
                hit = [k for k, (t, i) in enumerate(slots) if np.array_equal(boxes[b, t, i], row)]
                assert len(hit) == 1
                kept.append(slots[hit[0]])
            cnt = torch.bincount(inst, minlength=len(kept)).numpy()
            pooled = scatter_max(est.iou_estimator(feats), inst, 0)[0].numpy()
            iou = est.estimate(feats, inst).numpy()
            for k, (t, i) in enumerate(kept):
                ref_npts[b, t, i], ref_iou[b, t, i], ref_pooled[b, t, i] = cnt[k], iou[k], pooled[k]
            ref_survivors += [[i for (tt, i) in kept if tt == t] for t in range(NT)]
            # a sample of (point, box) feature rows: the first and last point of every surviving box
            start = np.concatenate([[0], np.cumsum(cnt)])
            for k, (t, i) in enumerate(kept):
                m = EN.inside(frames[b], boxes[b, t, i])
                idx = np.nonzero(m)[0]
                assert len(idx) == cnt[k]
                for which in (0, len(idx) - 1):
                    feat_pairs.append((b, t, i, int(idx[which])))
                    feat_ref.append(feats[start[k] + which].numpy())

    # ---- the restatement against the reference
    assert np.array_equal(y["npts"], ref_npts), "membership differs"
    assert y["survivors"] == ref_survivors, "survivors differ"
    gap = float(np.nanmax(np.abs(ref_iou.astype(np.float64) - y["iou"])))
    pooled_gap = float(np.abs(ref_pooled.astype(np.float64) - y["pooled"]).max())
    feat_y = np.stack([EN.features(frames[b][p:p + 1], boxes[b, t, i], labels[b, t, i], NC)[0] for b, t, i, p in feat_pairs])
    feat_gap = float(np.abs(np.stack(feat_ref).astype(np.float64) - feat_y).max())
    assert gap < 2e-6 and feat_gap < 1e-5 and pooled_gap < 1e-4, (gap, feat_gap, pooled_gap)
    # ---- the shapes the tests rely on
    n0 = y["npts"][0]
    assert n0[0, 2] == 1 and n0[0, 4] == 0 and n0[0, 5] == 1 and n0[0, 6] == 0 and n0[0, 7] == 0 and n0[1, 3] == 0
    assert n0[0, 0] > 10 and n0[0, 1] > 10 and n0[0, 3] >= 20
    both = EN.inside(frames[0], boxes[0, 0, 0]) & EN.inside(frames[0], boxes[0, 0, 1])
    assert both.sum() >= 5, "the overlapping boxes share no point"
    ring = EN.features(frames[0][EN.inside(frames[0], boxes[0, 0, 3])], boxes[0, 0, 3], 0, NC)[:, 3:5]
    assert (ring.min(axis=1) < 0).all(), "ring points with positive centerness"
    assert y["counts"][1].sum() == 0 and y["counts"][2].sum() == 0 and y["counts"][3].sum() == 0
    assert np.abs(boxes[..., 6]).max() > np.pi and boxes[..., 6].min() < 0 < boxes[..., 6].max()

    out = dict(boxes=boxes, scores=scores, labels=labels, counts=COUNTS, points=points, offsets=offsets,
               num_classes=np.int64(NC), task_classes=np.array([4, 6], dtype=np.int64),
               ref_npts=ref_npts, ref_iou=ref_iou, ref_pooled=ref_pooled, ref_out_counts=y["counts"],
               ref_survivor_mask=np.array([[[i in ref_survivors[b * NT + t] for i in range(POST)] for t in range(NT)]
                                           for b in range(B)]),
               f64_iou=y["iou"], f64_pooled=y["pooled"], feat_pairs=np.array(feat_pairs, dtype=np.int64),
               ref_features=np.stack(feat_ref), ref_f32_gap=np.float64(gap), ref_f32_pooled_gap=np.float64(pooled_gap),
               dropped_share=np.float64(share), margin=np.float64(MARGIN))
    out.update({"state." + k: v for k, v in state.items()})
    path = os.path.join(ROOT, "tests", "golden", "estimator.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; dropped {share:.3%}; ref_f32_gap {gap:.3e}; pooled gap "
          f"{pooled_gap:.3e} (max |pooled| {np.abs(y['pooled']).max():.3f}); feature gap {feat_gap:.3e}; "
          f"survivors {int(y['counts'].sum())}; points per box {y['npts'][0].tolist()}")


if __name__ == "__main__":
    main()
