"""Host restatements for the pre-pass tests (numpy float64; never imported by the product).

``match_frames`` restates classwise_weight/algo.py:36-106 per frame (the loop, the sort of :54, the strict ``<`` of :81,
``min_dist < dist_th`` of :86) with the devkit's published ``center_distance`` / ``scale_iou`` formulas, the range rule of
``filter_eval_boxes``, the per-match reductions of ppal_unc.py:76 and cald_ent.py:81-88, and the inverse of the augmented
view.  tests/test_prepass_host.py pins it to the reference's own ``accumulate`` through tests/golden/prepass_match.npz;
the edge cases of tests/test_prepass_gpu.py take their expected values from it.
"""
import numpy as np


def view_points(xyz, view):
    """det3d's flip / rotation / scaling of points (preprocess.py:787-854), float64."""
    fx, fy, rot, scale = view
    x = np.asarray(xyz[..., 0], np.float64) * (-1.0 if fy else 1.0)
    y = np.asarray(xyz[..., 1], np.float64) * (-1.0 if fx else 1.0)
    c, s = np.cos(rot), np.sin(rot)
    out = np.array(xyz, np.float64)
    out[..., 0] = (c * x + s * y) * scale
    out[..., 1] = (-s * x + c * y) * scale
    if out.shape[-1] > 2:
        out[..., 2] = np.asarray(xyz[..., 2], np.float64) * scale
    return out


def unview_xy(x, y, view):
    fx, fy, rot, scale = view
    c, s = np.cos(rot), np.sin(rot)
    xs, ys = x / scale, y / scale
    return (c * xs - s * ys) * (-1.0 if fy else 1.0), (s * xs + c * ys) * (-1.0 if fx else 1.0)


def scale_iou(sa, sr):
    sa, sr = np.asarray(sa, np.float64), np.asarray(sr, np.float64)
    inter = np.prod(np.minimum(sa, sr))
    return inter / (np.prod(sa) + np.prod(sr) - inter)


def match_frames(boxes, scores, labels, counts, ref_boxes, ref_labels, ref_scores, ref_off, ncls, dist_th=1.0,
                 class_range=None, origin=None, view=None):
    boxes, scores = np.asarray(boxes, np.float64), np.asarray(scores)
    ref_boxes = np.asarray(ref_boxes, np.float64).reshape(len(ref_labels), -1) if len(ref_labels) else np.zeros((0, 9))
    B, nt, post = scores.shape
    match_ref = np.full((B, nt, post), -1, np.int32)
    match_iou = np.zeros((B, nt, post), np.float64)
    cls_count = np.zeros((B, ncls), np.int32)
    cls_quality = np.zeros((B, ncls), np.float64)
    cls_cons = np.ones((B, ncls), np.float64)
    scale = 1.0 if view is None else float(view[3])
    for b in range(B):
        preds = []                                          # (t, i, x, y) in the frame's concatenated order
        for t in range(nt):
            for i in range(min(max(int(counts[b, t]), 0), post)):
                x, y = boxes[b, t, i, 0], boxes[b, t, i, 1]
                if view is not None:
                    x, y = unview_xy(x, y, view)
                preds.append((t, i, x, y))
        rows = list(range(int(ref_off[b]), int(ref_off[b + 1])))

        def in_range(x, y, c):
            return class_range is None or not np.hypot(x - origin[b][0], y - origin[b][1]) >= class_range[c]

        for c in range(ncls):
            cand = [(float(scores[b, t, i]), pos, t, i, x, y) for pos, (t, i, x, y) in enumerate(preds)
                    if labels[b, t, i] == c and in_range(x, y, c)]
            gts = [r for r in rows if ref_labels[r] == c and in_range(ref_boxes[r, 0], ref_boxes[r, 1], c)]
            taken = set()
            for s, _, t, i, x, y in sorted(cand, key=lambda v: (v[0], v[1]))[::-1]:
                best, hit = np.inf, None
                for r in gts:
                    if r in taken:
                        continue
                    d = np.linalg.norm(np.array([x, y]) - ref_boxes[r, :2])
                    if d < best:
                        best, hit = d, r
                if best < dist_th:
                    taken.add(hit)
                    iou = scale_iou(ref_boxes[hit, 3:6], boxes[b, t, i, 3:6] / scale)
                    match_ref[b, t, i], match_iou[b, t, i] = hit, iou
                    cls_count[b, c] += 1
                    cls_quality[b, c] += (s ** 0.6) * (iou ** 0.4)
                    p = float(ref_scores[hit])
                    cls_cons[b, c] = min(cls_cons[b, c], abs(iou + 0.5 * (p + s) - 1.3))
    return dict(match_ref=match_ref, match_iou=match_iou, cls_count=cls_count, cls_quality=cls_quality, cls_cons=cls_cons)


def frame_arrays(frame, cls, score, iou, ref_score, num_frames, ncls):
    """Flat per-match records (as the reference's ``dict_p_iou`` holds them, frame by frame) -> the per-frame arrays of the
    matching kernel, float64: ``cls_count``, ``cls_quality`` (ppal_unc.py:76), ``cls_cons`` (cald_ent.py:81-88, js = 0)."""
    cnt = np.zeros((num_frames, ncls), np.int64)
    qual = np.zeros((num_frames, ncls), np.float64)
    cons = np.ones((num_frames, ncls), np.float64)
    for f, c, q, u, p in zip(frame, cls, score, iou, ref_score):
        cnt[f, c] += 1
        qual[f, c] += (float(q) ** 0.6) * (float(u) ** 0.4)
        cons[f, c] = min(cons[f, c], abs(float(u) + 0.5 * (float(p) + float(q)) - 1.3))
    return cnt, qual, cons
