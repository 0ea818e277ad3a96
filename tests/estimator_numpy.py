"""Float64 restatement of the box-wise IoU estimator (the yardstick of tests/test_estimator_{cpu,gpu}.py), written from the
description of the semantics in INTEGRATION.md section 12; pure numpy, imports nothing from the package or the reference.

Layout as the kernel's: ``boxes [B,nt,post,D]``, ``labels [B,nt,post]``, ``counts [B,nt]``, ``points [P,F]``,
``offsets [B+1]``; ``state``: the module's state dict as numpy arrays."""
import numpy as np

ROT_COL = 6
BN_EPS = 1e-5


def footprint(box, rot_col=ROT_COL):
    """[4,2] corners of the doubled BEV footprint: local (-w,-l) (-w,l) (w,l) (w,-l), rotated CLOCKWISE by the angle
    (x' = x cos + y sin, y' = -x sin + y cos), moved to the centre."""
    x, y, w, l, r = (float(box[0]), float(box[1]), float(box[3]), float(box[4]), float(box[rot_col]))
    loc = np.array([[-w, -l], [-w, l], [w, l], [w, -l]], dtype=np.float64)
    c, s = np.cos(r), np.sin(r)
    return np.stack([loc[:, 0] * c + loc[:, 1] * s + x, -loc[:, 0] * s + loc[:, 1] * c + y], axis=1)


def edge_cross(points_xy, poly):
    """[N,4]: for corner k with predecessor k-1, (P_k - P_{k-1}) x-component times (P_k - p) y-component minus the
    y-component times the x-component; a point is inside iff all four are > 0."""
    prev = np.roll(poly, 1, axis=0)
    e = poly - prev                                         # [4,2]
    v = poly[None, :, :] - points_xy[:, None, :]            # [N,4,2]
    return e[None, :, 0] * v[:, :, 1] - e[None, :, 1] * v[:, :, 0]


def edge_distance(points_xy, poly):
    """[N] distance of every point to the nearest of the polygon's four edge SEGMENTS."""
    a = np.roll(poly, 1, axis=0)[None]                      # [1,4,2]
    d = (poly[None] - a)
    t = ((points_xy[:, None, :] - a) * d).sum(-1) / np.maximum((d * d).sum(-1), 1e-300)
    near = a + np.clip(t, 0.0, 1.0)[..., None] * d
    return np.sqrt(((points_xy[:, None, :] - near) ** 2).sum(-1)).min(axis=1)


def inside(points, box, rot_col=ROT_COL):
    """[N] bool: strictly inside the doubled footprint and |pz - z| <= h / 2 (the box's own height)."""
    p = np.asarray(points, dtype=np.float64)
    bev = (edge_cross(p[:, :2], footprint(box, rot_col)) > 0).all(axis=1)
    return bev & (np.abs(p[:, 2] - float(box[2])) <= float(box[5]) / 2)


def features(points, box, label, num_classes, rot_col=ROT_COL):
    """[n, 9 + num_classes]: the offset from the centre in the frame x' = dx cos + dy sin, y' = -dx sin + dy cos (the
    OTHER sense than the footprint's), the six centerness values on the un-expanded sizes, the label's one-hot."""
    p = np.asarray(points, dtype=np.float64)[:, :3]
    b = np.asarray(box, dtype=np.float64)
    d = p - b[None, :3]
    c, s = np.cos(b[rot_col]), np.sin(b[rot_col])
    loc = np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c, d[:, 2]], axis=1)
    hw, hl, hh = b[3] / 2, b[4] / 2, b[5] / 2
    cen = np.stack([hw + loc[:, 0], hw - loc[:, 0], hl + loc[:, 1], hl - loc[:, 1], hh + loc[:, 2], hh - loc[:, 2]], axis=1)
    hot = np.zeros((len(p), num_classes), dtype=np.float64)
    hot[:, int(label)] = 1.0
    return np.concatenate([loc, cen, hot], axis=1)


def _block(x, state, prefix, i, bn=True):
    w = state[f"{prefix}.{i}.weight"].astype(np.float64)
    x = x @ w.T + state[f"{prefix}.{i}.bias"].astype(np.float64)
    if bn:
        j = i + 1
        g, beta = state[f"{prefix}.{j}.weight"].astype(np.float64), state[f"{prefix}.{j}.bias"].astype(np.float64)
        m, v = state[f"{prefix}.{j}.running_mean"].astype(np.float64), state[f"{prefix}.{j}.running_var"].astype(np.float64)
        x = np.maximum((x - m) / np.sqrt(v + BN_EPS) * g + beta, 0.0)
    return x


def point_net(feats, state):
    x = feats
    for i in (0, 3, 6):
        x = _block(x, state, "iou_estimator", i)
    return x


def head(pooled, state):
    x = _block(_block(pooled, state, "iou_head", 0), state, "iou_head", 3)
    x = _block(x, state, "iou_head", 6, bn=False)
    return 1.0 / (1.0 + np.exp(-x[..., 0]))


def run(boxes, labels, counts, points, offsets, state, num_classes, rot_col=ROT_COL):
    """-> dict(npts [B,nt,post] i64, pooled [B,nt,post,128] f64 (0 where no point), iou [B,nt,post] f64 (NaN where no
    point), counts [B,nt] i64, survivors: list over (b, t) of the kept slot indices, ascending)."""
    B, nt, post = labels.shape
    npts = np.zeros((B, nt, post), dtype=np.int64)
    pooled = np.zeros((B, nt, post, 128), dtype=np.float64)
    iou = np.full((B, nt, post), np.nan, dtype=np.float64)
    out_counts = np.zeros((B, nt), dtype=np.int64)
    survivors = []
    for b in range(B):
        pts = np.asarray(points[int(offsets[b]):int(offsets[b + 1])], dtype=np.float64)
        for t in range(nt):
            keep = []
            for i in range(min(max(int(counts[b, t]), 0), post)):
                m = inside(pts, boxes[b, t, i], rot_col) if len(pts) else np.zeros((0,), dtype=bool)
                npts[b, t, i] = int(m.sum())
                if npts[b, t, i] == 0:
                    continue
                f = features(pts[m], boxes[b, t, i], labels[b, t, i], num_classes, rot_col)
                pooled[b, t, i] = point_net(f, state).max(axis=0)
                iou[b, t, i] = head(pooled[b, t, i][None], state)[0]
                keep.append(i)
            survivors.append(keep)
            out_counts[b, t] = len(keep)
    return dict(npts=npts, pooled=pooled, iou=iou, counts=out_counts, survivors=survivors)


def frame_entropy(scores):
    """Mean binary entropy of a frame's scores (entropy_selector.py:72-75); NaN for an empty frame."""
    p = np.asarray(scores, dtype=np.float64)
    if p.size == 0:
        return float("nan")
    return float((-p * np.log(p) - (1 - p) * np.log(1 - p)).mean())
