"""Float64 numpy restatement of the anchor head's post-processing for one (sample, task): the yardstick of the anchor-head
GPU tests (tests/test_anchorhead_fp64_gpu.py), itself pinned to the reference's own ``predict`` golden
(tests/test_anchorhead_fp64_cpu.py).  No project code; the polygon geometry is center_fp64's.

Semantics (det3d/models/bbox_heads/mg_head.py:697-803,981-1063, det3d/core/bbox/box_torch_ops.py:80-148,
det3d/ops/nms/nms_cpu.h:73-168): second_box_decode with the angle vector, sigmoid scores, best class = first argmax, keep
``score >= score_thresh``, order by score (equal scores: the lower anchor index first -- the device rule; torch.topk leaves it
open), the best ``pre_max`` enter the NMS, sequential greedy rotated NMS that stops at ``post_max`` survivors -- a later box
falls when the stand-up boxes overlap strictly, the intersection and the union are positive and ``inter / union >= thr``
(``>=``, CenterPoint's rule is ``>``) -- and the ``post_center_limit_range`` mask on the survivors, order kept.
"""
import numpy as np

from center_fp64 import clip_area, corners


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def decode(enc, anchors):
    """second_box_decode, encode_angle_to_vector=True: enc [n,10], anchors [n,9] (x y z w l h vx vy r) -> [n,9]."""
    t, a = np.asarray(enc, np.float64).reshape(-1, 10), np.asarray(anchors, np.float64).reshape(-1, 9)
    diag = np.sqrt(a[:, 4] ** 2 + a[:, 3] ** 2)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([t[:, 0] * diag + a[:, 0], t[:, 1] * diag + a[:, 1], t[:, 2] * a[:, 5] + a[:, 2],
                         np.exp(t[:, 3]) * a[:, 3], np.exp(t[:, 4]) * a[:, 4], np.exp(t[:, 5]) * a[:, 5],
                         t[:, 6] + a[:, 6], t[:, 7] + a[:, 7],
                         np.arctan2(t[:, 9] + np.sin(a[:, 8]), t[:, 8] + np.cos(a[:, 8]))], axis=1)


def select(cls_logits, score_thresh, pre_max):
    """cls_logits [A, nc] -> (anchor indices in rank order, their scores, their labels)."""
    s = sigmoid(cls_logits)
    top, lab = s.max(1), s.argmax(1)                     # argmax: the first of equal maxima
    idx = np.nonzero(top >= score_thresh)[0]             # NaN scores compare false
    order = idx[np.lexsort((idx, -top[idx]))][:pre_max]
    return order, top[order], lab[order]


def standup(c):
    return c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max()


def _own_frame_overlap(cp, cq):
    """Area of (P) n (bounding box of Q in P's frame); P = rectangle with corners cp [4,2]: >= |P n Q|."""
    u, v = cp[3] - cp[0], cp[1] - cp[0]
    lu, lv = np.hypot(*u), np.hypot(*v)
    if not (lu > 0 and lv > 0):
        return np.nan
    m = 0.5 * (cp[0] + cp[2])
    a, b = (cq - m) @ (u / lu), (cq - m) @ (v / lv)
    ow = min(a.max(), 0.5 * lu) - max(a.min(), -0.5 * lu)
    oh = min(b.max(), 0.5 * lv) - max(b.min(), -0.5 * lv)
    return max(ow, 0.0) * max(oh, 0.0)


def pair_quantities(a, b, ca=None, cb=None):
    """a, b = (x, y, w, l, r) -> dict(iou, inter, standup_overlap, and the upper bounds of the IoU that the kernel's
    prefilters use: ``ratio`` = min / max of the areas, ``standup`` = o / (A + B - o) of the stand-up overlap o, ``own_a`` /
    ``own_b`` = the same with the overlap in a's / b's own frame).  iou is None when the stand-up boxes do not overlap
    strictly (the pair is never clipped) or the areas are not numbers."""
    ca, cb = corners(*a) if ca is None else ca, corners(*b) if cb is None else cb
    sa, sb = standup(ca), standup(cb)
    iw, ih = min(sa[2], sb[2]) - max(sa[0], sb[0]), min(sa[3], sb[3]) - max(sa[1], sb[1])
    q = dict(iou=None, inter=0.0, standup_overlap=0.0)
    if not (iw > 0 and ih > 0):
        return q
    A, B = a[2] * a[3], b[2] * b[3]
    if not (np.isfinite(ca).all() and np.isfinite(cb).all()):
        return q
    inter = clip_area(ca - ca[0], cb - ca[0])            # about a's first corner: the yardstick's own shoelace stays exact-ish at range
    uni = A + B - inter
    ub = lambda o: o / (A + B - o) if A + B - o > 0 else np.inf      # noqa: E731
    q.update(inter=inter, standup_overlap=iw * ih, iou=inter / uni if (inter > 0 and uni > 0) else 0.0,
             ratio=min(A, B) / max(A, B) if max(A, B) > 0 else np.inf, standup=ub(iw * ih),
             own_a=ub(_own_frame_overlap(ca, cb)), own_b=ub(_own_frame_overlap(cb, ca)))
    return q


def rotate_nms(bev, thr, post_max, pairs=None, strict=False):
    """bev [n,5] in rank order -> kept indices.  ``pairs`` collects (i, j, quantities) of every evaluated pair whose
    stand-up boxes overlap.  ``strict=True`` is the WRONG rule (``>``), kept for the demonstration that the tests tell
    the two apart."""
    n = len(bev)
    alive = np.ones(n, bool)
    keep = []
    with np.errstate(invalid="ignore"):
        cs = np.stack([corners(*b) for b in bev]) if n else np.zeros((0, 4, 2))
        lo, hi = cs.min(1), cs.max(1)                    # stand-up boxes; NaN corners give NaN, which compares false below
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) == post_max:
            break
        with np.errstate(invalid="ignore"):
            meet = ((np.minimum(hi[i], hi) - np.maximum(lo[i], lo)) > 0).all(1) & alive
        for j in np.nonzero(meet[i + 1:])[0] + i + 1:
            q = pair_quantities(bev[i], bev[j], cs[i], cs[j])
            if q["iou"] is None:
                continue
            if pairs is not None:
                pairs.append((i, j, q))
            if q["iou"] > 0 and (q["iou"] > thr if strict else q["iou"] >= thr):
                alive[j] = False
    return keep


def task_predict(hout, anchors, na, nc, box_off, cls_off, score_thresh, iou_thresh, pre_max, post_max, rng, pairs=None,
                 strict=False):
    """hout [HW, CH] of one sample, anchors [HW * na, 9] of one task -> dict(anchors = kept anchor indices in output order,
    boxes [k,9], scores, labels (without the task's label offset), cand = anchor indices that entered the NMS in rank order,
    cand_boxes, nms_keep = ranks that survived the NMS, before the range mask)."""
    hout = np.asarray(hout)
    hw = hout.shape[0]
    order, score, label = select(hout[:, cls_off:cls_off + na * nc].reshape(hw * na, nc), score_thresh, pre_max)
    boxes = decode(hout[:, box_off:box_off + na * 10].reshape(hw * na, 10)[order], np.asarray(anchors).reshape(-1, 9)[order])
    keep = np.asarray(rotate_nms(boxes[:, [0, 1, 3, 4, 8]], iou_thresh, post_max, pairs, strict), np.int64)
    r = np.asarray(rng, np.float64)
    b = boxes[keep]
    nms_keep = keep
    keep = keep[(b[:, :3] >= r[:3]).all(1) & (b[:, :3] <= r[3:]).all(1)]     # NaN centres fail the mask
    return dict(anchors=order[keep], boxes=boxes[keep], scores=score[keep], labels=label[keep], cand=order, cand_boxes=boxes,
                nms_keep=nms_keep)
