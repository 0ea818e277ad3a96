"""TEST INFRASTRUCTURE ONLY.  Golden vectors for the anchor head with the direction classifier and the scalar / 7-dim box codes
(tests/golden/head_predict_codes.npz): the reference's own ``MultiGroupHead.predict`` (det3d/models/bbox_heads/mg_head.py:
697-803) -> ``GroundBox3dCoderTorch.decode_torch`` (box_coders.py:106-109) -> ``get_task_detections`` (mg_head.py:805-1085)
with ``use_direction_classifier``, called unbound on seeded head outputs.  ``import_head`` and ``_Cfg`` are those of
oracle/gen_golden_head_predict.py, so the compiled ``rotate_nms_cc`` is this build's oracle here exactly as it is there.
Needs the reference tree; run in the build container only:  python tools/gen_golden_anchor_head_codes.py

Cases (n_dim, vector code, classifier, direction_offset): see ``CASES``.  Shape: B = 2, an 8 x 8 map, two tasks with
(nc 1, na 2) and (nc 2, na 4), pre_max 64 and post_max 16 (both cuts bite), a centre range that drops border boxes, and one
(sample, task) with every class logit at -20.

A float32 decision must not sit on an edge, so each case's seed is redrawn until THE REFERENCE'S OWN numbers keep clear of
every edge (``check_bands``; no case is dropped, the seed found is recorded in the file):
  * scores (torch.sigmoid) of a (sample, task) that pass the threshold are pairwise >= 1e-5 apart, and every score is >= 1e-4
    from the threshold;
  * every decoded |r - direction_offset| >= 1e-3 (decode_torch on all anchors);
  * the two direction logits of every anchor differ by >= 1e-3;
  * every pair the NMS evaluates has an IoU outside anchorhead_cases.DELTA["origin"] of the threshold.
"""
import functools
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden", "head_predict_codes.npz")
B, H, W = 2, 8, 8
NUM_CLASSES = [1, 2]
SCORE_THR, IOU_THR, PRE_MAX, POST_MAX = 0.1, 0.2, 64, 16
RANGE = [-11.0, -11.0, -10.0, 11.0, 11.0, 10.0]
EMPTY = (1, 1)                                       # (sample, task) with every class logit at -20
# name: (n_dim, vec_encode, classifier, direction_offset)
CASES = {"s7_dir": (7, False, True, 0.78), "s9_dir": (9, False, True, 0.0), "v7_dir": (7, True, True, 0.78),
         "s9_nodir": (9, False, False, 0.0), "v9_dir": (9, True, True, 0.0)}
# (class, w-l-h, z): task 0 one class, task 1 two
CLASSES = [[("car", [1.97, 4.63, 1.74], -0.95)], [("motorcycle", [0.77, 2.11, 1.47], -1.085), ("bicycle", [0.60, 1.70, 1.28], -1.18)]]


def task_anchors(n_dim):
    from al3d.datasets.anchors import generate_task_anchors
    tasks = [dict(num_class=len(g), class_names=[c[0] for c in g]) for g in CLASSES]
    gens = []
    for g in CLASSES:
        for name, size, z in g:
            d = dict(class_name=name, sizes=size, anchor_ranges=[-12.8, -12.8, z, 12.8, 12.8, z], rotations=[0, 1.57])
            if n_dim == 9:
                d["velocities"] = [0, 0]
            gens.append(d)
    out = generate_task_anchors(tasks, gens, [1, H, W])
    assert all(a.shape == (H * W * 2 * nc, n_dim) for a, nc in zip(out, NUM_CLASSES))
    return out


def draw(seed, n_dim, vec, with_dir):
    rng = np.random.default_rng(seed)
    code = n_dim + int(vec)
    box, cls, dirs = [], [], []
    for t, nc in enumerate(NUM_CLASSES):
        na = 2 * nc
        box.append(rng.normal(0.0, 0.3, (B, H, W, na * code)).astype(np.float32))
        c = rng.normal(-1.0, 2.0, (B, H, W, na * nc)).astype(np.float32)
        if t == EMPTY[1]:
            c[EMPTY[0]] = -20.0
        cls.append(c)
        dirs.append(rng.normal(0.0, 1.0, (B, H, W, na * 2)).astype(np.float32) if with_dir else None)
    return box, cls, dirs


def check_bands(bto, box, cls, dirs, anchors, n_dim, vec, offset, out=None):
    """-> None when the reference's own numbers keep clear of every edge, else the name of the first edge met."""
    import anchorhead_cases as AC
    import head_fp64 as HF
    code = n_dim + int(vec)
    cuts = 0
    for t, nc in enumerate(NUM_CLASSES):
        for b in range(B):
            s = torch.sigmoid(torch.from_numpy(cls[t][b]).view(-1, nc)).numpy().astype(np.float64)
            if np.abs(s - np.float64(np.float32(SCORE_THR))).min() < 1e-4:
                return "score on the threshold"
            top = np.sort(s.max(1)[s.max(1) >= SCORE_THR])
            if len(top) > 1 and np.diff(top).min() < 1e-5:
                return "two candidate scores closer than 1e-5"
            dec = bto.second_box_decode(torch.from_numpy(box[t][b]).view(-1, code), torch.from_numpy(anchors[t]), vec, False)
            dec = dec.numpy().astype(np.float64)
            if np.abs(dec[:, -1] - np.float64(np.float32(offset))).min() < 1e-3:
                return "angle on the direction offset"
            if dirs[t] is not None:
                d = dirs[t][b].reshape(-1, 2).astype(np.float64)
                if np.abs(d[:, 1] - d[:, 0]).min() < 1e-3:
                    return "direction logits closer than 1e-3"
            if (b, t) == EMPTY:
                if len(top):
                    return "the empty (sample, task) has a candidate"
                continue
            order, _, _ = HF.select(cls[t][b].reshape(-1, nc), np.float64(np.float32(SCORE_THR)), PRE_MAX)
            pairs = []
            keep = HF.rotate_nms(dec[order][:, [0, 1, 3, 4, -1]], np.float64(np.float32(IOU_THR)), POST_MAX, pairs)
            if any(abs(q["iou"] - np.float64(np.float32(IOU_THR))) < AC.DELTA["origin"] for _, _, q in pairs):
                return "IoU on the threshold"
            if not (len(top) > PRE_MAX and len(keep) == POST_MAX):
                return "a cut does not bite"
            cuts += 1
    assert cuts == 2 * B - 1
    return None


def reference_predict(mg, coders, box, cls, dirs, anchors, n_dim, vec, with_dir, offset):
    from gen_golden_head_predict import _Cfg
    coder = coders.GroundBox3dCoderTorch(linear_dim=False, vec_encode=vec, n_dim=n_dim, norm_velo=False)
    head = types.SimpleNamespace(use_direction_classifier=with_dir, direction_offset=offset, encode_background_as_zeros=True,
                                 use_sigmoid_score=True, num_anchor_per_locs=[2 * c for c in NUM_CLASSES],
                                 num_classes=NUM_CLASSES, anchor_dim=n_dim, bev_only=False, box_n_dim=coder.code_size,
                                 box_coder=coder)
    head.get_task_detections = functools.partial(mg.MultiGroupHead.get_task_detections, head)
    cfg = _Cfg(score_threshold=SCORE_THR, post_center_limit_range=RANGE,
               nms=_Cfg(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=PRE_MAX, nms_post_max_size=POST_MAX,
                        nms_iou_threshold=IOU_THR))
    preds = []
    for t in range(len(NUM_CLASSES)):
        d = {"box_preds": torch.from_numpy(box[t].copy()), "cls_preds": torch.from_numpy(cls[t].copy())}
        if with_dir:
            d["dir_cls_preds"] = torch.from_numpy(dirs[t].copy())
        preds.append(d)
    example = {"voxels": None, "num_points": None, "coordinates": None,
               "anchors": [torch.from_numpy(np.broadcast_to(a, (B,) + a.shape).copy()) for a in anchors]}
    with torch.no_grad():
        return mg.MultiGroupHead.predict(head, example, preds, cfg)


def main():
    import oracle
    import ref_import
    from gen_golden_head_predict import import_head
    oracle.build()
    mg, bto = import_head()
    ref_import.import_box_np_ops()
    coders = importlib.import_module("det3d.core.bbox.box_coders")
    store = {"shape": np.array([B, H, W], np.int64), "num_classes": np.array(NUM_CLASSES, np.int64),
             "params": np.array([SCORE_THR, IOU_THR, PRE_MAX, POST_MAX], np.float64), "range": np.array(RANGE, np.float64),
             "cases": np.array(sorted(CASES))}
    for k, (name, (n_dim, vec, with_dir, offset)) in enumerate(sorted(CASES.items())):
        anchors = task_anchors(n_dim)
        seed, why = 1000 * (k + 1), "not drawn"
        while why is not None:
            seed += 1
            box, cls, dirs = draw(seed, n_dim, vec, with_dir)
            why = check_bands(bto, box, cls, dirs, anchors, n_dim, vec, offset)
        out = reference_predict(mg, coders, box, cls, dirs, anchors, n_dim, vec, with_dir, offset)
        assert check_bands(bto, box, cls, dirs, anchors, n_dim, vec, offset) is None
        store[f"{name}.cfg"] = np.array([n_dim, int(vec), int(with_dir), offset, seed], np.float64)
        for t in range(len(NUM_CLASSES)):
            store.update({f"{name}.box{t}": box[t], f"{name}.cls{t}": cls[t], f"{name}.anchors{t}": anchors[t]})
            if with_dir:
                store[f"{name}.dir{t}"] = dirs[t]
        for b in range(B):
            store.update({f"{name}.out{b}.boxes": out[b]["box3d_lidar"].numpy(), f"{name}.out{b}.scores": out[b]["scores"].numpy(),
                          f"{name}.out{b}.labels": out[b]["label_preds"].numpy()})
            assert out[b]["box3d_lidar"].shape[1] == n_dim
        print(name, "seed", seed, "->", [tuple(o["box3d_lidar"].shape) for o in out],
              "labels", [np.bincount(o["label_preds"].numpy(), minlength=3).tolist() for o in out])
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
