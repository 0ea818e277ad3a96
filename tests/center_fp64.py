"""Float64 numpy restatement of the CenterPoint post-processing: the yardstick of the CenterHead GPU tests, itself pinned to
the reference coder's golden (tests/test_centerhead_golden.py).

Semantics (bevfusion/mmdet3d/models/heads/bbox/centerpoint.py:637-884, core/bbox/coders/centerpoint_bbox_coders.py:62-225,
ops/iou3d/src/iou3d_kernel.cu:159-169,244-250,326, core/post_processing/box3d_nms.py:180-219): per class the K best cells,
the K best of those, class = candidate // K; equal scores: the smaller ``class * D0 * D1 + cell`` wins (the device rule;
torch.topk leaves it open).  Maps are ``[C, D0, D1]``; ``swapped=False``: x runs along D0 and y along D1 (the
reference's [x, y] maps), ``swapped=True``: the other way round.
"""
import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def topk(score, K):
    """score [C, D0, D1] -> (scores [K], class [K], cell [K]) in descending score order."""
    C = score.shape[0]
    hw = score.shape[1] * score.shape[2]
    flat = score.reshape(C, hw)
    cand_s, cand_i = [], []
    for c in range(C):
        order = np.lexsort((np.arange(hw), -flat[c]))[:K]
        cand_s.append(flat[c, order])
        cand_i.append(c * hw + order)
    cand_s, cand_i = np.concatenate(cand_s), np.concatenate(cand_i)
    order = np.lexsort((cand_i, -cand_s))[:K]
    return cand_s[order], cand_i[order] // hw, cand_i[order] % hw


def decode(score, reg, hei, dim, rot, vel, *, K, swapped, out_size_factor, voxel_size, pc_range, score_threshold,
           post_center_range):
    """CenterPointBBoxCoder.decode for one sample.  score [C,D0,D1]; reg [2,..] or None; hei [1,..]; dim [3,..] (already
    exp'ed when norm_bbox); rot [2,..] = (sine, cosine); vel [2,..] or None.
    -> dict(boxes [n,9|7], scores, labels, cells, all_boxes [K, .], all_scores [K]) of the survivors, in score order."""
    D1 = score.shape[2]
    s, cls, cell = topk(np.asarray(score, np.float64), K)
    d0, d1 = cell // D1, cell % D1
    xs, ys = (d1, d0) if swapped else (d0, d1)
    g = lambda m, k: np.asarray(m, np.float64)[k].reshape(-1)[cell]      # noqa: E731
    xs = xs + (g(reg, 0) if reg is not None else 0.5)
    ys = ys + (g(reg, 1) if reg is not None else 0.5)
    x = xs * out_size_factor * voxel_size[0] + pc_range[0]
    y = ys * out_size_factor * voxel_size[1] + pc_range[1]
    cols = [x, y, g(hei, 0), g(dim, 0), g(dim, 1), g(dim, 2), np.arctan2(g(rot, 0), g(rot, 1))]
    if vel is not None:
        cols += [g(vel, 0), g(vel, 1)]
    boxes = np.stack(cols, axis=1)
    r = np.asarray(post_center_range, np.float64)
    mask = (boxes[:, :3] >= r[:3]).all(1) & (boxes[:, :3] <= r[3:]).all(1)
    if score_threshold:
        mask &= s > score_threshold
    return dict(boxes=boxes[mask], scores=s[mask], labels=cls[mask], cells=cell[mask], all_boxes=boxes, all_scores=s,
                all_labels=cls, all_cells=cell, mask=mask)


def corners(x, y, w, l, r):
    """xywhr2xyxyr + the kernel's rotation about the centre: [4, 2]."""
    c, s = np.cos(r), np.sin(r)
    px = np.array([-0.5, -0.5, 0.5, 0.5]) * w
    py = np.array([-0.5, 0.5, 0.5, -0.5]) * l
    return np.stack([px * c + py * s + x, -px * s + py * c + y], axis=1)


def clip_area(a, b):
    """Area of the intersection of two convex quadrilaterals [4,2] (Sutherland-Hodgman + shoelace)."""
    poly = [tuple(p) for p in a]
    area_b = sum(b[k][0] * b[(k + 1) % 4][1] - b[(k + 1) % 4][0] * b[k][1] for k in range(4))
    sgn = 1.0 if area_b >= 0 else -1.0
    for e in range(4):
        if not poly:
            break
        bx, by = b[e]
        ex, ey = b[(e + 1) % 4][0] - bx, b[(e + 1) % 4][1] - by
        out = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            dp = sgn * (ex * (p[1] - by) - ey * (p[0] - bx))
            dq = sgn * (ex * (q[1] - by) - ey * (q[0] - bx))
            if dp >= 0:
                out.append(p)
            if (dp >= 0) != (dq >= 0):
                t = dp / (dp - dq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = out
    if len(poly) < 3:
        return 0.0
    return 0.5 * abs(sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[(k + 1) % len(poly)][0] * poly[k][1]
                         for k in range(len(poly))))


def bev_iou(a, b):
    """a, b = (x, y, w, l, r): iou_bev (overlap / max(sa + sb - overlap, 1e-8))."""
    if np.hypot(a[0] - b[0], a[1] - b[1]) > 0.5 * (np.hypot(a[2], a[3]) + np.hypot(b[2], b[3])):
        return 0.0
    inter = clip_area(corners(*a), corners(*b))
    return inter / max(a[2] * a[3] + b[2] * b[3] - inter, 1e-8)


def rotate_nms(bev, thr, post_max, pairs=None):
    """bev [n,5] in score order -> kept indices; a later box is suppressed when IoU > thr (strict).  ``pairs`` collects
    (i, j, iou) of every evaluated pair with a positive IoU."""
    n = len(bev)
    alive = np.ones(n, bool)
    keep = []
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) == post_max:
            break
        for j in range(i + 1, n):
            if alive[j]:
                iou = bev_iou(bev[i], bev[j])
                if pairs is not None and iou > 0:
                    pairs.append((i, j, iou))
                if iou > thr:
                    alive[j] = False
    return keep


def circle_nms(xy, radius, post_max, pairs=None):
    """xy [n,2] in score order -> kept indices; a later one is suppressed when its squared distance <= radius."""
    n = len(xy)
    alive = np.ones(n, bool)
    keep = []
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) == post_max:
            break
        d2 = (xy[i + 1:, 0] - xy[i, 0]) ** 2 + (xy[i + 1:, 1] - xy[i, 1]) ** 2
        if pairs is not None:
            pairs.extend((i, i + 1 + int(j), float(d2[j])) for j in np.nonzero(alive[i + 1:])[0])
        alive[i + 1:] &= ~(d2 <= radius)
    return keep


def task_detections(dec, *, nms_type, nms_scale, min_radius, score_threshold, nms_thr, pre_max_size, post_max_size,
                    post_center_limit_range, pairs=None):
    """The NMS stage of one (sample, task) on ``decode``'s survivors -> indices into them, in kept order."""
    boxes, scores, labels = dec["boxes"], dec["scores"], dec["labels"]
    if nms_type == "circle":
        return np.asarray(circle_nms(boxes[:, :2], min_radius, post_max_size, pairs), np.int64)
    idx = np.arange(len(scores))
    if score_threshold > 0.0:
        idx = idx[scores >= score_threshold]
    idx = idx[:pre_max_size]
    sc = np.asarray(nms_scale, np.float64)[labels[idx]]
    bev = np.stack([boxes[idx, 0], boxes[idx, 1], boxes[idx, 3] * sc, boxes[idx, 4] * sc, boxes[idx, 6]], axis=1)
    keep = idx[np.asarray(rotate_nms(bev, nms_thr, post_max_size, pairs), np.int64)]
    if post_center_limit_range is not None and len(post_center_limit_range):
        r = np.asarray(post_center_limit_range, np.float64)
        b = boxes[keep]
        keep = keep[(b[:, :3] >= r[:3]).all(1) & (b[:, :3] <= r[3:]).all(1)]
    return keep


def postprocess(hout, task_ncls, chan_off, *, swapped, max_num, norm_bbox, out_size_factor, voxel_size, pc_range,
                coder_score_threshold, post_center_range, nms_type, nms_scale, min_radius, score_threshold, nms_thr,
                pre_max_size, post_max_size, post_center_limit_range, merge=True, pairs=None):
    """The arguments of ``al3d.detector_ops.center_decode_nms`` on a numpy ``hout`` [B,D0,D1,CH] ->
    [[dict(boxes, scores, labels, cells) per task] per sample]; ``pairs[(b, t)]`` collects the NMS pair quantities."""
    h = np.asarray(hout, np.float64)
    B = h.shape[0]
    kinds = [nms_type] * len(task_ncls) if isinstance(nms_type, str) else list(nms_type)
    out = []
    for b in range(B):
        row, label_off = [], 0
        for t, ncls in enumerate(task_ncls):
            heat, reg, hei, dim, rot, vel = chan_off[t]
            m = lambda o, n: None if o < 0 else np.moveaxis(h[b, :, :, o:o + n], 2, 0)      # noqa: E731
            d = m(dim, 3)
            dec = decode(sigmoid(m(heat, ncls)), m(reg, 2), m(hei, 1), np.exp(d) if norm_bbox else d, m(rot, 2), m(vel, 2),
                         K=max_num, swapped=swapped, out_size_factor=out_size_factor, voxel_size=voxel_size, pc_range=pc_range,
                         score_threshold=coder_score_threshold, post_center_range=post_center_range)
            pl = None if pairs is None else pairs.setdefault((b, t), [])
            keep = task_detections(dec, nms_type=kinds[t], nms_scale=nms_scale[t], min_radius=min_radius[t],
                                   score_threshold=score_threshold, nms_thr=nms_thr, pre_max_size=pre_max_size,
                                   post_max_size=post_max_size, post_center_limit_range=post_center_limit_range, pairs=pl)
            boxes = dec["boxes"][keep].copy()
            if vel < 0:
                boxes = np.concatenate([boxes, np.zeros((len(boxes), 2))], axis=1)
            labels = dec["labels"][keep].copy()
            if merge:
                boxes[:, 2] -= boxes[:, 5] * 0.5
                labels += label_off
            row.append(dict(boxes=boxes, scores=dec["scores"][keep], labels=labels, cells=dec["cells"][keep], decoded=dec))
            label_off += ncls
        out.append(row)
    return out
