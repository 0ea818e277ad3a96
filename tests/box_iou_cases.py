"""Inputs, float64 yardsticks and the measured float32 band of the box IoU / NMS ops (csrc/box_iou.hip): shared by
tests/test_box_iou_cpu.py and tests/test_box_iou_gpu.py.  No project code; the polygon geometry is center_fp64's.

YARDSTICKS.  ``metric_matrix`` on ``inter_matrix64``: float64 exact clipping of the two footprints (about a's first corner,
as head_fp64 does) put through the metric's formula.  ``nms64``: a float64 greedy loop over those IoUs (only pairs that can
meet are stored) in the device's candidate order (descending score, NaN last, equal scores by the lower index).
``best64``: the row maximum with the lowest row among equal maxima.  A row with a non-finite number or a footprint size
that is not positive is not a box (``is_box``): 0 with everything, the rule of include/al3d.h.

BOXES.  Rows are ``[x, y, z, s0, s1, h, r]`` float32; "det3d" turns the corners by -r (rotation_2d), "heading" by +r.
``plants(shift)`` builds the named families -- identical, edge_touch, corner_touch, inside, right_angles (k pi/2 against
k pi/2 +- 1e-4), sliver (1 cm wide), zero_size, far -- and ``matrix_pool`` repeats them at the origin and at (+-54, +-54) m
and pads with random traffic boxes, so that the sizes {0, 1, T-1, T, T+1, 2T+1} of both tile edges (16 rows, 64 columns)
are slices of one pool with one yardstick.

THE BAND IS MEASURED, NOT CHOSEN.  ``measure`` takes every pair these cases evaluate and forms, with the float32 CPU oracle
(``oracle.rbox_pair``; never the kernel), max |IoU_f32 - IoU_f64| per family (``MEASURED``; "random" are the pool's
other overlapping pairs, "best" / "nms" the pairs of those cases, "golden" the pairs of tests/golden/box_iou_eval.npz).  The oracle has the BEV IoU only:
for the other metrics the oracle's float32 intersection area and the float32 areas of its own float32 corners are put
through the metric's formula in float64, with the volumes and the height overlap rounded to float32 as the kernel forms
them, and the result is recorded per metric (``MEASURED_METRIC``; overlaps are m^2 / m^3, the rest are ratios).  The
assertion bound is 4 x the recorded maximum: the project's allowance for device sinf / cosf differing from libm by an ulp
per corner (tests/anchorhead_cases.py).  ``python tests/box_iou_cases.py`` reprints the figures; tests/test_box_iou_cpu.py
fails when a recomputed maximum exceeds its record or falls below 0.8 of it.  Re-record by copying the printed figures,
rounded up to two digits.

DECISION BAND.  Keep lists and ``best_ref`` must equal the yardstick exactly, so no generated pair may have a float64 IoU
within ``BAND`` of the threshold, and no row two maxima within ``BAND`` of each other unless the reference rows are exact
duplicates.  Offenders are redrawn; the redrawn share is recorded in the case and asserted < 1 %.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from center_fp64 import clip_area, corners  # noqa: E402

T_ROWS, T_COLS = 16, 64
SIZES_N = (0, 1, T_ROWS - 1, T_ROWS, T_ROWS + 1, 2 * T_ROWS + 1)
SIZES_M = (0, 1, T_COLS - 1, T_COLS, T_COLS + 1, 2 * T_COLS + 1)
METRICS = ("overlap", "iou", "over_a", "over_b")
HEIGHTS = ("_bev", "3d", "3d_kitti")
CONVENTIONS = ("det3d", "heading")
PLACEMENTS = ((0.0, 0.0), (54.0, 54.0), (-54.0, 54.0), (54.0, -54.0), (-54.0, -54.0))
FOOT = ((0.41, 0.41), (0.67, 0.73), (0.60, 1.70), (0.77, 2.11), (2.53, 0.50), (1.97, 4.63), (2.51, 6.93), (2.94, 10.5))
NMS_THR = 0.3

# max |IoU_f32 - IoU_f64| of the BEV IoU per family, both conventions and the xyxyr rows (module docstring)
MEASURED = {"identical": 1.7e-14, "edge_touch": 0.0, "corner_touch": 0.0, "inside": 1.3e-07,
            "right_angles": 3.2e-07, "sliver": 7.3e-07, "zero_size": 0.0, "far": 0.0, "random": 1.9e-06,
            "best": 1.4e-06, "nms": 1.5e-06, "golden": 4.2e-06}
# the same error put through every metric's formula, over all pairs
MEASURED_METRIC = {"iou3d": 6.0e-06, "iou3d_kitti": 6.0e-06, "iou_bev": 4.2e-06, "over_a3d": 1.3e-04,
                   "over_a3d_kitti": 1.3e-04, "over_a_bev": 1.1e-04, "over_b3d": 1.9e-04, "over_b3d_kitti": 1.9e-04,
                   "over_b_bev": 1.1e-04, "overlap3d": 5.4e-05, "overlap3d_kitti": 5.1e-05, "overlap_bev": 2.9e-05}
BAND = 4.0 * max(MEASURED.values())
BAND_METRIC = {k: 4.0 * v for k, v in MEASURED_METRIC.items()}
# what an exact decision (a keep list, a best row) must stay clear of: the widest band of the IoUs that decide
BAND_DECIDE = max(BAND, BAND_METRIC.get("iou3d", 0.0))


# ---------------------------------------------------------------- float64 geometry
def corners64(row, convention):
    x, y, _, s0, s1, _, r = (float(v) for v in row)
    return corners(x, y, s0, s1, r if convention == "det3d" else -r)


def inter64(ca, cb):
    return clip_area(ca - ca[0], cb - ca[0])


def apart(a, b, slack=1e-9):
    """[n, m] bool: the bounding circles are apart in float64 -- such a pair's intersection is exactly empty"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1])
    ra, rb = 0.5 * np.hypot(a[:, 3], a[:, 4]), 0.5 * np.hypot(b[:, 3], b[:, 4])
    return d > (ra[:, None] + rb[None, :]) * (1 + slack) + 1e-300


def inter_matrix64(a, b, convention, pairs=None):
    """Footprint intersection areas [n, m] in float64; rows with a non-finite entry give 0.  ``pairs``: only these (i, j)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros((len(a), len(b)))
    if not len(a) or not len(b):
        return out
    fa, fb = np.isfinite(a).all(1), np.isfinite(b).all(1)
    with np.errstate(invalid="ignore"):
        near = ~apart(np.where(fa[:, None], a, 0.0), np.where(fb[:, None], b, 0.0)) & fa[:, None] & fb[None, :]
    ca = [corners64(r, convention) if fa[i] else None for i, r in enumerate(a)]
    cb = [corners64(r, convention) if fb[j] else None for j, r in enumerate(b)]
    for i, j in (zip(*np.nonzero(near)) if pairs is None else pairs):
        if near[i, j]:
            out[i, j] = inter64(ca[i], cb[j])
    return out


def is_box(rows):
    """[n] bool: every number finite and both footprint sizes positive; any other row gives 0 with everything"""
    rows = np.asarray(rows, np.float64).reshape(-1, 7)
    with np.errstate(invalid="ignore"):
        return np.isfinite(rows).all(1) & (rows[:, 3] > 0) & (rows[:, 4] > 0)


def zrange(rows, height):
    rows = np.asarray(rows, np.float64)
    if height == "3d_kitti":
        return rows[:, 2] - rows[:, 5], rows[:, 2]
    return rows[:, 2] - 0.5 * rows[:, 5], rows[:, 2] + 0.5 * rows[:, 5]


def metric_matrix(inter, a, b, metric, height, sa=None, sb=None, f32=False):
    """The metric's formula on footprint intersections [n, m].  ``f32``: volumes and the height overlap rounded to float32
    the way the kernel forms them (for the error propagation); sa / sb: footprint areas to use instead of s0 * s1."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = is_box(a)[:, None] & is_box(b)[None, :]
    a, b = np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0), np.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0)
    sa = a[:, 3] * a[:, 4] if sa is None else sa
    sb = b[:, 3] * b[:, 4] if sb is None else sb
    eps = 1e-8
    inter = np.array(inter, np.float64)
    if height != "_bev":
        if f32:
            r = lambda v: np.asarray(v, np.float32)                                     # noqa: E731
            a32, b32 = r(a), r(b)
            if height == "3d_kitti":
                la, ha, lb, hb = a32[:, 2] - a32[:, 5], a32[:, 2], b32[:, 2] - b32[:, 5], b32[:, 2]
            else:
                la, ha = a32[:, 2] - r(0.5) * a32[:, 5], a32[:, 2] + r(0.5) * a32[:, 5]
                lb, hb = b32[:, 2] - r(0.5) * b32[:, 5], b32[:, 2] + r(0.5) * b32[:, 5]
            hov = np.maximum(np.minimum(ha[:, None], hb[None, :]) - np.maximum(la[:, None], lb[None, :]), r(0)).astype(np.float64)
            sa, sb = (a32[:, 3] * a32[:, 4] * a32[:, 5]).astype(np.float64), (b32[:, 3] * b32[:, 4] * b32[:, 5]).astype(np.float64)
        else:
            (la, ha), (lb, hb) = zrange(a, height), zrange(b, height)
            hov = np.maximum(np.minimum(ha[:, None], hb[None, :]) - np.maximum(la[:, None], lb[None, :]), 0.0)
            sa, sb = a[:, 3] * a[:, 4] * a[:, 5], b[:, 3] * b[:, 4] * b[:, 5]
        inter = inter * hov
        eps = 1e-6
    sa, sb = np.broadcast_to(np.asarray(sa)[:, None], inter.shape), np.broadcast_to(np.asarray(sb)[None, :], inter.shape)
    if metric == "overlap":
        v = inter
    elif metric == "iou":
        v = inter / np.maximum(sa + sb - inter, eps)
    elif metric == "over_a":
        v = inter / np.maximum(sa, eps)
    else:
        v = inter / np.maximum(sb, eps)
    return np.where(ok, v, 0.0)


def xyxyr_rows(rows):
    """[n, 7] -> the float32 [x1, y1, x2, y2, r] rows of xywhr2xyxyr and the float64 7-rows those float32 numbers mean"""
    rows = np.asarray(rows, np.float32)
    h0, h1 = rows[:, 3] / np.float32(2), rows[:, 4] / np.float32(2)
    x = np.stack([rows[:, 0] - h0, rows[:, 1] - h1, rows[:, 0] + h0, rows[:, 1] + h1, rows[:, 6]], 1).astype(np.float32)
    x64 = x.astype(np.float64)
    z = np.zeros(len(x))
    mean = np.stack([0.5 * (x64[:, 0] + x64[:, 2]), 0.5 * (x64[:, 1] + x64[:, 3]), z, x64[:, 2] - x64[:, 0], x64[:, 3] - x64[:, 1], z,
                     x64[:, 4]], 1)
    return x, mean


# ---------------------------------------------------------------- the matrix pool
def _row(x, y, s0, s1, r, z=-0.9, h=1.6):
    return [x, y, z, s0, s1, h, r]


def plants(shift=(0.0, 0.0)):
    """-> [(family, a row, b row)]: what the families claim is checked in float64 by tests/test_box_iou_cpu.py"""
    px, py = shift
    out = [("identical", _row(px + 1, py + 2, 1.97, 4.63, 0.3), _row(px + 1, py + 2, 1.97, 4.63, 0.3)),
           ("identical", _row(px - 3, py, 0.67, 0.73, -2.0, z=0.2, h=1.8), _row(px - 3, py, 0.67, 0.73, -2.0, z=0.2, h=1.8)),
           ("edge_touch", _row(px, py, 2.0, 4.0, 0.0), _row(px + 2.0, py, 2.0, 4.0, 0.0, z=-0.5)),
           ("corner_touch", _row(px, py, 2.0, 4.0, 0.0), _row(px + 2.0, py + 4.0, 2.0, 4.0, 0.0)),
           ("inside", _row(px + 0.5, py, 4.0, 6.0, 0.2, h=2.0), _row(px + 0.5, py, 1.0, 2.0, 0.9, z=-0.7, h=1.0)),
           ("sliver", _row(px, py + 1, 0.01, 6.0, 0.1), _row(px + 0.25, py + 1, 1.97, 4.63, -0.4, z=-0.2)),
           ("sliver", _row(px, py - 1, 0.01, 6.0, 0.1), _row(px, py - 1, 0.01, 6.0, 0.1 + 0.5)),
           ("zero_size", _row(px, py, 0.0, 0.0, 0.5), _row(px, py, 1.97, 4.63, 0.0)),
           ("zero_size", _row(px, py, 0.0, 4.0, 0.5), _row(px, py, 0.0, 4.0, 0.5)),
           ("far", _row(px, py, 1.97, 4.63, 0.3), _row(px + 20.0, py + 10.0, 1.97, 4.63, 0.3))]
    for k in range(4):
        for sgn in (-1.0, 1.0):
            out.append(("right_angles", _row(px, py, 1.97, 4.63, k * np.pi / 2, z=-1 + 0.1 * k),
                        _row(px + 0.5, py + 0.3, 1.97, 4.63, k * np.pi / 2 + sgn * 1e-4, z=-0.8)))
    return [(f, np.asarray(a, np.float32), np.asarray(b, np.float32)) for f, a, b in out]


def random_boxes(rng, n, spread=6.0):
    """n traffic boxes clustered around the five placements"""
    place = np.asarray(PLACEMENTS)[rng.integers(0, len(PLACEMENTS), n)]
    foot = np.asarray(FOOT)[rng.integers(0, len(FOOT), n)] * rng.uniform(0.8, 1.2, (n, 1))
    return np.concatenate([place + rng.uniform(-spread, spread, (n, 2)), rng.uniform(-1.5, 0.0, (n, 1)), foot,
                           rng.uniform(1.0, 2.5, (n, 1)), rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)


_cache = {}


def matrix_pool():
    """dict(a [NA,7], b [NB,7] float32, family [n_plants]): plant k is the pair (a[k], b[k]); NA >= 2 T_ROWS + 1 and
    NB >= 2 T_COLS + 1 after the random padding.  The first rows interleave the families so that small slices see them."""
    if "pool" not in _cache:
        ps = [p for shift in PLACEMENTS for p in plants(shift)]
        order = np.random.default_rng(7).permutation(len(ps))
        ps = [ps[i] for i in order]
        rng = np.random.default_rng(11)
        a = np.stack([p[1] for p in ps])
        b = np.stack([p[2] for p in ps])
        b = np.concatenate([b, random_boxes(rng, 2 * T_COLS + 1 + 8 - len(b))])
        _cache["pool"] = dict(a=a, b=b, family=[p[0] for p in ps])
    return _cache["pool"]


def matrix_yardstick(kind):
    """kind: "det3d" | "heading" | "xyxyr" -> dict(inter [NA,NB] float64, a, b float64 rows the yardstick used, a32, b32 the
    float32 rows the kernel gets)"""
    key = ("yard", kind)
    if key not in _cache:
        p = matrix_pool()
        if kind == "xyxyr":
            a32, a = xyxyr_rows(p["a"])
            b32, b = xyxyr_rows(p["b"])
            conv = "det3d"
        else:
            a32, b32, a, b, conv = p["a"], p["b"], p["a"].astype(np.float64), p["b"].astype(np.float64), kind
        _cache[key] = dict(inter=inter_matrix64(a, b, conv), a=a, b=b, a32=a32, b32=b32, convention=conv)
    return _cache[key]


def nonfinite_rows(rows, which, rng):
    """a copy of float32 rows with a NaN or an inf planted in the rows ``which`` (one column each, cycling x .. r)"""
    out = np.array(rows, np.float32)
    for k, i in enumerate(which):
        out[i, k % out.shape[1]] = (np.nan, np.inf, -np.inf)[k % 3]
    return out


# ---------------------------------------------------------------- the float32 oracle's error
def oracle_pair(oracle, a, b, convention):
    """float32 rows -> (intersection area, IoU, area a, area b): the oracle's float32 results; the areas are those of its own
    float32 corners (shoelace about the first corner, in float64)"""
    sgn = 1.0 if convention == "det3d" else -1.0
    a5 = np.asarray([a[0], a[1], a[3], a[4], sgn * a[6]], np.float32)
    b5 = np.asarray([b[0], b[1], b[3], b[4], sgn * b[6]], np.float32)
    ca, cb, inter, iou = oracle.rbox_pair(a5, b5)

    def area(c):
        x, y = c[:4].astype(np.float64) - float(c[0]), c[4:].astype(np.float64) - float(c[4])
        return 0.5 * abs(sum(x[k] * y[k + 1] - x[k + 1] * y[k] for k in (1, 2)))
    return inter, iou, area(ca), area(cb)


def measure_pairs(oracle, a32, b32, a64, b64, inter, convention, pairs, iou_err, metric_err, family):
    """Fold the pairs (i, j) into ``iou_err[family(i, j)]`` (BEV IoU, the oracle's own) and ``metric_err[metric + height]``"""
    in32, iou32, mask = np.zeros_like(inter), np.zeros_like(inter), np.zeros(inter.shape, bool)
    sa32, sb32 = np.zeros(len(a32)), np.zeros(len(b32))
    for i, j in pairs:
        if is_box(_seven(a32[i]))[0] and is_box(_seven(b32[j]))[0]:
            in32[i, j], iou32[i, j], sa32[i], sb32[j] = oracle_pair(oracle, _seven(a32[i]), _seven(b32[j]), convention)
            mask[i, j] = True
    if not mask.any():
        return
    err = np.abs(iou32 - metric_matrix(inter, a64, b64, "iou", "_bev"))
    for i, j in zip(*np.nonzero(mask)):
        f = family(i, j)
        iou_err[f] = max(iou_err.get(f, 0.0), float(err[i, j]))
    for m in METRICS:
        for h in HEIGHTS:
            e = np.abs(metric_matrix(in32, a64, b64, m, h, sa=sa32, sb=sb32, f32=True) - metric_matrix(inter, a64, b64, m, h))
            metric_err[m + h] = max(metric_err.get(m + h, 0.0), float(e[mask].max()))


def _seven(row):
    """a float32 row of 5 (xyxyr) or >= 7 columns -> the 7 numbers (x, y, z, s0, s1, h, r) in float32 arithmetic"""
    row = np.asarray(row, np.float32)
    if len(row) == 5:
        return np.asarray([np.float32(0.5) * (row[0] + row[2]), np.float32(0.5) * (row[1] + row[3]), 0, row[2] - row[0],
                           row[3] - row[1], 0, row[4]], np.float32)
    return np.concatenate([row[:6], row[-1:]]) if len(row) != 7 else row


def measure(oracle):
    """-> (MEASURED, MEASURED_METRIC) recomputed over every pair the cases evaluate with a positive intersection, and
    every planted pair"""
    iou_err, metric_err = {}, {}
    p = matrix_pool()
    n_pl = len(p["family"])
    for kind in ("det3d", "heading", "xyxyr"):
        y = matrix_yardstick(kind)
        near = np.nonzero(y["inter"] > 0)
        pairs = sorted(set(zip(near[0].tolist(), near[1].tolist())) | {(k, k) for k in range(n_pl)})
        measure_pairs(oracle, y["a32"], y["b32"], y["a"], y["b"], y["inter"], y["convention"], pairs, iou_err, metric_err,
                      lambda i, j: p["family"][i] if i == j and i < n_pl else "random")
    c = best_case()
    for b in range(c["B"]):
        sl = slice(c["ref_off"][b], c["ref_off"][b + 1])
        pred = c["boxes"][b].reshape(-1, c["boxes"].shape[-1])
        p7 = np.concatenate([pred[:, :6], pred[:, -1:]], 1)
        measure_pairs(oracle, p7, c["ref_boxes"][sl], p7.astype(np.float64), c["ref_boxes"][sl].astype(np.float64), c["inter"][b],
                      "det3d", list(zip(*np.nonzero(c["inter"][b] > 0))), iou_err, metric_err, lambda i, j: "best")
    for name in NMS_CASES:
        c = nms_case(name)
        if c["inter"] is None:
            continue
        b64 = c["boxes"].astype(np.float64)
        measure_pairs(oracle, c["boxes"], c["boxes"], b64, b64, c["inter"], c["convention"],
                      [(i, j) for i, j in zip(*np.nonzero(c["inter"] > 0)) if i < j], iou_err, metric_err, lambda i, j: "nms")
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_iou_eval.npz"))
    diag = [(i, i) for i in range(len(z["boxes"]))]
    pad = lambda b: np.stack([b[:, 0], b[:, 1], 0 * b[:, 0], b[:, 2], b[:, 3], 0 * b[:, 0], b[:, 4]], 1)      # noqa: E731
    cam = lambda b: np.stack([b[:, 0], b[:, 2], b[:, 1], b[:, 3], b[:, 5], b[:, 4], b[:, 6]], 1)               # noqa: E731
    for a32, b32 in ((pad(z["boxes"]), pad(z["query"])), (cam(z["cam_boxes"]), cam(z["cam_query"]))):
        a64, b64 = a32.astype(np.float64), b32.astype(np.float64)
        measure_pairs(oracle, a32, b32, a64, b64, inter_matrix64(a64, b64, "det3d", pairs=diag), "det3d", diag, iou_err, metric_err,
                      lambda i, j: "golden")
    for f in MEASURED:
        iou_err.setdefault(f, 0.0)
    return iou_err, metric_err


# ---------------------------------------------------------------- best IoU per detection
def best64(iou, ref_labels=None, labels=None):
    """iou [n, m] -> (max [n], lowest row among equal maxima [n]); with labels only the rows of the slot's class.  0 / -1
    where no row."""
    n, m = iou.shape
    val, ref = np.zeros(n), np.full(n, -1, np.int64)
    for i in range(n):
        cand = np.arange(m) if labels is None else np.nonzero(ref_labels == labels[i])[0]
        if len(cand):
            k = cand[np.argmax(iou[i, cand])]                  # argmax: the first of equal maxima
            val[i], ref[i] = iou[i, k], k
    return val, ref


def best_case():
    """B = 3 frames, nt = 3 tasks, post = 5 slots, 9-column boxes (angle last), 7-column references.  counts: frame 0
    (0, 1, post), frame 1 (post + 2, -2, 1), frame 2 (post, post, 0); reference rows: 3 * 64 + 1, 0 and 1.  Frame 0's slot
    (2, 0) has its best row in the last reference tile (row 192), slot (2, 1) overlaps the exact duplicates 10 and 70."""
    if "best" in _cache:
        return _cache["best"]
    rng = np.random.default_rng(23)
    B, nt, post = 3, 3, 5
    counts = np.array([[0, 1, post], [post + 2, -2, 1], [post, post, 0]], np.int32)
    nref = [3 * T_COLS + 1, 0, 1]
    ref_off = np.concatenate([[0], np.cumsum(nref)]).astype(np.int32)
    R = int(ref_off[-1])
    # references of frame 0 on a 14 x 14 grid of 6 m cells: a detection meets a few of them
    cells = rng.permutation(14 * 14)[:nref[0]]
    ref = np.zeros((R, 7), np.float32)
    ref[:nref[0], 0] = (cells % 14 - 7) * 6.0 + rng.uniform(-0.5, 0.5, nref[0])
    ref[:nref[0], 1] = (cells // 14 - 7) * 6.0 + rng.uniform(-0.5, 0.5, nref[0])
    ref[:, 2] = rng.uniform(-1.2, -0.6, R)
    ref[:, 3:5] = np.asarray(FOOT)[rng.integers(3, 7, R)]
    ref[:, 5] = rng.uniform(1.4, 2.0, R)
    ref[:, 6] = rng.uniform(-np.pi, np.pi, R)
    ref[70] = ref[10]                                          # exact duplicates: the lower row wins
    ref[R - 1, :2] = (3.0, -2.0)                               # frame 2's only row
    ref_labels = rng.integers(0, 3, R).astype(np.int32)
    ref_labels[70] = ref_labels[10]
    boxes = np.zeros((B, nt, post, 9), np.float32)
    labels = rng.integers(0, 3, (B, nt, post)).astype(np.int32)
    target = rng.integers(0, nref[0], (B, nt, post))
    target[0, 2, 0], target[0, 2, 1] = nref[0] - 1, 10
    target[2] = R - 1
    redrawn = total = 0
    inter = [None] * B
    for b in range(B):
        sl = slice(ref_off[b], ref_off[b + 1])
        for t in range(nt):
            for s in range(post):
                while True:
                    total += 1
                    src = ref[target[b, t, s]]
                    row = np.array(src, np.float64)
                    row[:2] += rng.uniform(-0.8, 0.8, 2)
                    row[2] += rng.uniform(-0.2, 0.2)
                    row[3:6] *= rng.uniform(0.85, 1.15, 3)
                    row[6] += rng.uniform(-0.3, 0.3)
                    boxes[b, t, s, :6], boxes[b, t, s, 8] = row[:6], row[6]
                    boxes[b, t, s, 6:8] = rng.uniform(-3, 3, 2)        # velocities: never read
                    if nref[b] == 0:
                        break
                    p7 = np.concatenate([boxes[b, t, s, :6], boxes[b, t, s, 8:]])[None].astype(np.float64)
                    r64 = ref[sl].astype(np.float64)
                    ok = True
                    for h in ("_bev", "3d"):
                        iou = metric_matrix(inter_matrix64(p7, r64, "det3d"), p7, r64, "iou", h)[0]
                        for cand in [np.arange(len(iou))] + [np.nonzero(ref_labels[sl] == c)[0] for c in range(3)]:
                            top = cand[iou[cand] >= iou[cand].max(initial=0.0) - 2 * BAND_DECIDE]      # rows that could win
                            if len(top) > 1 and iou[cand].max() > 0 and not (b == 0 and set(top.tolist()) <= {10, 70}):
                                ok = False
                    if ok:
                        break
                    redrawn += 1
        p = boxes[b].reshape(-1, 9)
        p7 = np.concatenate([p[:, :6], p[:, 8:]], 1).astype(np.float64)
        inter[b] = inter_matrix64(p7, ref[sl].astype(np.float64), "det3d")
    _cache["best"] = dict(B=B, nt=nt, post=post, counts=counts, boxes=boxes, labels=labels, ref_boxes=ref, ref_labels=ref_labels,
                          ref_off=ref_off, inter=inter, redrawn_share=redrawn / total)
    return _cache["best"]


def best_yardstick(case, metric, height, same_class):
    """-> (best_iou [B,nt,post] float64, best_ref [B,nt,post] int64 rows of ref_boxes)"""
    B, nt, post = case["B"], case["nt"], case["post"]
    val, ref = np.zeros((B, nt * post)), np.full((B, nt * post), -1, np.int64)
    for b in range(B):
        r0, r1 = case["ref_off"][b], case["ref_off"][b + 1]
        p = case["boxes"][b].reshape(-1, 9)
        p7 = np.concatenate([p[:, :6], p[:, 8:]], 1).astype(np.float64)
        iou = metric_matrix(case["inter"][b], p7, case["ref_boxes"][r0:r1].astype(np.float64), metric, height)
        v, k = best64(iou, case["ref_labels"][r0:r1] if same_class else None, case["labels"][b].reshape(-1) if same_class else None)
        valid = (np.arange(post)[None, :] < np.clip(case["counts"][b], 0, post)[:, None]).reshape(-1)
        val[b] = np.where(valid & (k >= 0), v, 0.0)
        ref[b] = np.where(valid & (k >= 0), k + r0, -1)
    return val.reshape(B, nt, post), ref.reshape(B, nt, post)


# ---------------------------------------------------------------- NMS
def score_order(scores):
    """candidate order of csrc/al3d_sort_key.h: descending, NaN last, -0 == +0, equal scores by the lower index"""
    s = np.asarray(scores, np.float64)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), -np.where(nan, 0.0, s), nan))


def normal_iou64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    w = np.minimum(a[0] + a[3] / 2, b[0] + b[3] / 2) - np.maximum(a[0] - a[3] / 2, b[0] - b[3] / 2)
    h = np.minimum(a[1] + a[4] / 2, b[1] + b[4] / 2) - np.maximum(a[1] - a[4] / 2, b[1] - b[4] / 2)
    inter = max(w, 0.0) * max(h, 0.0)
    return inter / max(a[3] * a[4] + b[3] * b[4] - inter, 1e-8)


def _cluster_pool(rng, n, thresh, mode="rotated", convention="heading"):
    """n boxes in clusters of one to four on a 10 m grid (only boxes of one cluster can meet); pairs within BAND of the
    threshold are redrawn -> (boxes float32 [n,7], iou float64 [n,n] upper triangle, redrawn share)"""
    side = int(np.ceil(np.sqrt(n / 2.0))) + 1
    boxes = np.zeros((n, 7), np.float32)
    pairs = {}
    i = c = redrawn = total = 0
    while i < n:
        size = min(int(rng.integers(1, 5)), n - i)
        cx, cy = (c % side - side / 2) * 10.0, (c // side - side / 2) * 10.0
        for k in range(size):
            while True:
                total += 1
                foot = np.asarray(FOOT)[5] * rng.uniform(0.8, 1.2, 2)
                boxes[i] = [cx + rng.uniform(-1.2, 1.2), cy + rng.uniform(-1.2, 1.2), -1.0, foot[0], foot[1], 1.6,
                            rng.uniform(-np.pi, np.pi)]
                vals = {}
                for j in range(i - k, i):
                    if mode == "normal":
                        vals[j] = normal_iou64(boxes[j], boxes[i])
                    else:
                        a, b = boxes[j:j + 1].astype(np.float64), boxes[i:i + 1].astype(np.float64)
                        vals[j] = metric_matrix(inter_matrix64(a, b, convention), a, b, "iou", "_bev")[0, 0]
                if all(abs(v - thresh) > BAND_DECIDE for v in vals.values()):
                    break
                redrawn += 1
            for j, v in vals.items():
                pairs[(j, i)] = v
            i += 1
        c += 1
    return boxes, pairs, redrawn / max(total, 1)


NMS_CASES = ("chain", "duplicates", "pre_max_ties", "post_max", "nan_score", "normal", "n0", "n1", "n64", "n65", "n4096",
             "n4097_pre4096")


def nms_case(name):
    """-> dict(boxes [n,7] float32, scores [n] float32, thresh, pre_max, post_max, mode, convention, expect = kept indices of
    the float64 loop, inter [n,n] float64 footprint intersections (n <= 300), n, redrawn_share)"""
    key = ("nms", name)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(sum(map(ord, name)))
    c = dict(thresh=NMS_THR, pre_max=None, post_max=None, mode="rotated", convention="heading", redrawn_share=0.0)
    car = lambda x, y, r=0.0: _row(x, y, 2.0, 4.0, r)          # noqa: E731
    if name == "chain":        # along x: IoU(A,B) = IoU(B,C) = 1/3 > 0.3, IoU(A,C) = 0: A kills B, C lives
        c.update(boxes=[car(0, 0), car(1.0, 0), car(2.0, 0), car(30, 0)], scores=[0.9, 0.8, 0.7, 0.6])
    elif name == "duplicates":
        c.update(boxes=[car(5, 5, 0.4), car(0, 0, 0.3), car(0, 0, 0.3), car(5, 5, 0.4)], scores=[0.5, 0.7, 0.7, 0.5])
    elif name == "pre_max_ties":
        c.update(boxes=[car(10 * k, 0) for k in range(6)], scores=[0.5, 0.9, 0.5, 0.5, 0.5, 0.1], pre_max=3)
    elif name == "post_max":
        c.update(boxes=[car(10 * k, 0) for k in range(6)] + [car(0.2, 0)], scores=[0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.85], post_max=3)
    elif name == "nan_score":
        c.update(boxes=[car(0, 0), car(0.1, 0), car(20, 0), car(20.1, 0), car(40, 0)], scores=[np.nan, 0.2, 0.6, np.nan, -0.0])
    else:
        n = {"normal": 40, "n0": 0, "n1": 1, "n64": 64, "n65": 65, "n4096": 4096, "n4097_pre4096": 4097}[name]
        if name == "normal":
            c["mode"] = "normal"
        if name == "n4097_pre4096":
            c["pre_max"] = 4096
        boxes, pairs, share = _cluster_pool(rng, n, NMS_THR, c["mode"], c["convention"])
        scores = rng.permutation(n).astype(np.float32) / np.float32(max(n, 1))
        if n >= 64:
            scores[5] = scores[40]                                  # one tie between clusters far apart
        c.update(boxes=boxes, scores=scores, pairs=pairs, redrawn_share=share)
    boxes = np.asarray(c["boxes"], np.float32).reshape(-1, 7)
    scores = np.asarray(c["scores"], np.float32).reshape(-1)
    n = len(boxes)
    if "pairs" in c:
        pairs = c.pop("pairs")
    else:
        pairs = {}
        b64 = boxes.astype(np.float64)
        im = inter_matrix64(b64, b64, c["convention"])
        io = metric_matrix(im, b64, b64, "iou", "_bev")
        for i in range(n):
            for j in range(i + 1, n):
                pairs[(i, j)] = normal_iou64(boxes[i], boxes[j]) if c["mode"] == "normal" else io[i, j]
    iou = _SparseIou(pairs)
    inter = None
    if n <= 300 and c["mode"] == "rotated":
        b64 = boxes.astype(np.float64)
        inter = inter_matrix64(b64, b64, c["convention"])
    c.update(boxes=boxes, scores=scores, n=n, inter=inter, pair_iou=pairs,
             expect=nms64(iou, scores, c["thresh"], c["pre_max"], c["post_max"]))
    _cache[key] = c
    return c


class _SparseIou:
    """IoU of the pairs that can meet; every other pair is 0"""

    def __init__(self, pairs):
        self.nb = {}
        for (i, j), v in pairs.items():
            self.nb.setdefault(i, []).append((j, v))
            self.nb.setdefault(j, []).append((i, v))


def nms64(iou, scores, thresh, pre_max=None, post_max=None):
    """The float64 greedy loop over a _SparseIou -> kept input indices, in candidate order"""
    order = score_order(scores)
    if pre_max is not None and pre_max > 0:
        order = order[:pre_max]
    rank = {int(i): p for p, i in enumerate(order)}
    dead, keep = set(), []
    for pos, i in enumerate(order):
        i = int(i)
        if i in dead:
            continue
        keep.append(i)
        if post_max is not None and post_max > 0 and len(keep) == post_max:
            break
        for j, v in iou.nb.get(i, ()):
            if j in rank and rank[j] > pos and v > thresh:
                dead.add(j)
    return np.asarray(keep, np.int64)


LAUNCH_MATRIX = ((1, 64, 1), (7, 128, 1), (16, 64, 1), (128, 256, 1), (16, 256, 0))          # tile_rows, threads, reject
LAUNCH_BEST = ((1, 1, 64, 1), (5, 64, 128, 1), (128, 17, 256, 1), (3, 64, 256, 1), (128, 64, 256, 0))      # chunk, ref_tile, threads, reject
LAUNCH_NMS = ((256, 64, 1), (1024, 128, 1), (256, 256, 0))                                    # sort, mask threads, reject


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import oracle
    oracle.build()
    iou_err, metric_err = measure(oracle)
    print("MEASURED = {" + ", ".join(f'"{f}": {iou_err[f]:.2e}' for f in MEASURED) + "}")
    print("MEASURED_METRIC = {" + ", ".join(f'"{m}": {v:.2e}' for m, v in sorted(metric_err.items())) + "}")
    print("best redrawn", best_case()["redrawn_share"], {n: nms_case(n)["redrawn_share"] for n in NMS_CASES})
