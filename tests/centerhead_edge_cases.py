"""Hand-built inputs that sit ON the decisions of the CenterHead post-processing kernel (csrc/center_head.hip), shared by
the CPU check of the cases (tests/test_centerhead_edge_cases_cpu.py) and the GPU test (tests/test_centerhead_edges_gpu.py).
numpy only.  tests/centerhead_cases.py keeps its inputs off every threshold; these put them on it, which needs every
compared quantity to be EXACT in float32, so that the float32 kernel and the float64 yardstick decide alike:

  * geometry: out_size_factor 8, voxel 0.125 m, integer pc_range: a cell is 1 m, ``reg`` offsets are binary fractions,
    so centres, corners, squared distances and axis-aligned overlaps are small dyadic rationals;
  * ``norm_bbox=False``: dimensions are the raw integers; ``rot = (0, 1)``: atan2 gives exactly 0; the height is copied;
  * scores: logit 0 -> exactly 0.5, -inf -> exactly 0 (the background), +inf -> exactly 1; equal logits tie; ordered
    scores come from logits k * 2^-12 (or from scores 0.5 + k * 2^-14), at least 1e-5 apart against a float32 sigmoid
    error of 2.4e-7, and equal in their two leading key bytes;
  * a threshold is put one float32 ulp either side of the exact value with ``below`` / ``above``.

``case(name)`` -> dict(h [B,D0,D1,CH] f32, task_ncls, chan, p (the keywords of ``center_decode_nms``), expect, h_nan).
``expect[b][t]`` is the hand-written answer: the kept (cell, class) pairs in output order, stated from the construction
and never from a run.  ``h_nan`` (non-finite family only) is ``h`` with NaN in place of some -inf heat logits: the device
must treat both alike.  ``expected_rows`` turns ``expect`` into boxes, scores and labels by gathering the inputs.
"""
import functools

import numpy as np

from centerhead_cases import layout

f32 = np.float32
# mirrors of csrc/center_head.hip's defines (compared in tests/test_centerhead_edge_cases_cpu.py)
LIMITS = dict(CT_THREADS=1024, CT_MAXK=1024, CT_MAXCAND=2048, CT_MAXPOST=512, CT_MAXCLS=4, CT_MAXTASKS=8)
WIDE = [-64.0, -64.0, -8.0, 64.0, 64.0, 8.0]
THR = 2.0 ** -10                    # default coder threshold: drops the background (0 > THR is false), keeps every plant


def below(v):
    return float(np.nextafter(f32(v), f32(-np.inf)))


def above(v):
    return float(np.nextafter(f32(v), f32(np.inf)))


def logit_k(k):
    return float(f32(k * 2.0 ** -12))


def logit_of(score):
    return float(f32(np.log(score / (1.0 - score))))


class Scene:
    """A head output whose every cell is background (heat -inf) with a unit box at the cell's middle; ``plant`` writes objects."""

    def __init__(self, D0, D1, task_ncls, B=1, swapped=True):
        self.D0, self.D1, self.task_ncls, self.swapped = D0, D1, list(task_ncls), swapped
        self.CH, self.chan = layout(self.task_ncls)
        self.h = np.zeros((B, D0 * D1, self.CH), f32)
        for t, n in enumerate(self.task_ncls):
            heat, reg, hei, dim, rot, vel = self.chan[t]
            self.h[:, :, heat:heat + n] = -np.inf
            self.h[:, :, reg:reg + 2] = 0.5
            self.h[:, :, dim:dim + 3] = 1.0
            self.h[:, :, rot + 1] = 1.0

    def cell(self, ix, iy):
        return iy * self.D1 + ix if self.swapped else ix * self.D1 + iy

    def plant(self, cell, logit, t=0, cls=0, b=0, reg=None, z=None, dim=None, vel=None):
        heat, r, hei, d, _, v = self.chan[t]
        self.h[b, cell, heat + cls] = logit
        if reg is not None:
            self.h[b, cell, r:r + 2] = reg
        if z is not None:
            self.h[b, cell, hei] = z
        if dim is not None:
            self.h[b, cell, d:d + 3] = dim
        if vel is not None:
            self.h[b, cell, v:v + 2] = vel
        return cell

    def map(self):
        return self.h.reshape(self.h.shape[0], self.D0, self.D1, self.CH).copy()

    def params(self, **over):
        nt = len(self.task_ncls)
        p = dict(swapped=self.swapped, max_num=8, norm_bbox=False, out_size_factor=8.0, voxel_size=[0.125, 0.125],
                 pc_range=[0.0, 0.0], coder_score_threshold=THR, post_center_range=WIDE, nms_type="circle",
                 nms_scale=[[1.0] * n for n in self.task_ncls], min_radius=[0.0] * nt, score_threshold=0.0, nms_thr=0.5,
                 pre_max_size=1000, post_max_size=16, post_center_limit_range=None, merge=True)
        p.update(over)
        return p

    def case(self, expect, **over):
        return dict(h=self.map(), task_ncls=self.task_ncls, chan=self.chan, p=self.params(**over), expect=expect, h_nan=None)


def expected_rows(c):
    """``expect`` -> [[dict(boxes [n,9] f64, scores f64, labels, cells, exact) per task] per sample], gathered from the
    inputs: every value is exact in float32 except the scores of logits other than 0 and +-inf (``exact`` marks the rest)."""
    h, p, chan = c["h"], c["p"], c["chan"]
    B, D0, D1, CH = h.shape
    assert p["out_size_factor"] * p["voxel_size"][0] == 1.0 == p["out_size_factor"] * p["voxel_size"][1] and not p["norm_bbox"]
    flat = h.reshape(B, D0 * D1, CH).astype(np.float64)
    out = []
    for b in range(B):
        row, off = [], 0
        for t, ncls in enumerate(c["task_ncls"]):
            heat, reg, hei, dim, rot, vel = chan[t]
            cells = np.array([e[0] for e in c["expect"][b][t]], np.int64)
            cls = np.array([e[1] for e in c["expect"][b][t]], np.int64)
            g = flat[b, cells]
            assert (g[:, rot] == 0).all() and (g[:, rot + 1] == 1).all()
            d0, d1 = cells // D1, cells % D1
            ix, iy = (d1, d0) if p["swapped"] else (d0, d1)
            z, dims = g[:, hei], g[:, dim:dim + 3]
            boxes = np.concatenate([np.stack([ix + g[:, reg] + p["pc_range"][0], iy + g[:, reg + 1] + p["pc_range"][1],
                                              z - dims[:, 2] / 2 if p["merge"] else z], 1), dims, np.zeros((len(cells), 1)),
                                    g[:, vel:vel + 2]], axis=1)
            logits = g[np.arange(len(cells)), heat + cls]
            with np.errstate(over="ignore"):
                scores = 1.0 / (1.0 + np.exp(-logits))
            row.append(dict(boxes=boxes, scores=scores, labels=cls + (off if p["merge"] else 0), cells=cells,
                            exact=(logits == 0) | np.isinf(logits)))
            off += ncls
        out.append(row)
    return out


def clip_area(ax, ay, bx, by, dt):
    """``quad_intersection_area`` of csrc/al3d_rbox.h, operation for operation, in the arithmetic ``dt``."""
    one, zero = dt(1), dt(0)
    px, py = [dt(v) for v in ax], [dt(v) for v in ay]
    bx, by = [dt(v) for v in bx], [dt(v) for v in by]
    barea = zero
    for k in range(4):
        k2 = (k + 1) & 3
        barea = dt(barea + dt(dt(bx[k] * by[k2]) - dt(bx[k2] * by[k])))
    sgn = one if barea >= 0 else -one
    for e in range(4):
        if not px:
            break
        e2 = (e + 1) & 3
        ex, ey = dt(bx[e2] - bx[e]), dt(by[e2] - by[e])
        qx, qy = [], []
        n = len(px)
        for k in range(n):
            k2 = 0 if k + 1 == n else k + 1
            d1 = dt(sgn * dt(dt(ex * dt(py[k] - by[e])) - dt(ey * dt(px[k] - bx[e]))))
            d2 = dt(sgn * dt(dt(ex * dt(py[k2] - by[e])) - dt(ey * dt(px[k2] - bx[e]))))
            if d1 >= 0:
                qx.append(px[k])
                qy.append(py[k])
            if (d1 >= 0) != (d2 >= 0):
                tt = dt(d1 / dt(d1 - d2))
                qx.append(dt(px[k] + dt(tt * dt(px[k2] - px[k]))))
                qy.append(dt(py[k] + dt(tt * dt(py[k2] - py[k]))))
        px, py = qx, qy
    if len(px) < 3:
        return zero
    area = zero
    for k in range(1, len(px) - 1):
        area = dt(area + dt(dt(dt(px[k] - px[0]) * dt(py[k + 1] - py[0])) - dt(dt(px[k + 1] - px[0]) * dt(py[k] - py[0]))))
    return dt(dt(0.5) * abs(area))


def axis_iou(a, b, dt):
    """IoU of two axis-aligned BEV boxes (x, y, w, l) as the kernel computes it (``box_corners`` at angle 0, the clip, the
    ``max(union, 1e-8)`` division) in the arithmetic ``dt``; a is the kept box (the clip's subject), b the later one."""
    def corners(q):
        x, y, w, l = [dt(v) for v in q]
        ux, uy = [-0.5, -0.5, 0.5, 0.5], [-0.5, 0.5, 0.5, -0.5]
        return [dt(dt(dt(u) * w) + x) for u in ux], [dt(dt(dt(u) * l) + y) for u in uy]
    (ax, ay), (bx, by) = corners(a), corners(b)
    inter = clip_area(ax, ay, bx, by, dt)
    union = dt(dt(dt(dt(a[2]) * dt(a[3])) + dt(dt(b[2]) * dt(b[3]))) - inter)
    return dt(inter / max(union, dt(1e-8)))


# the pairs of the rotated-NMS cases: (kept box, later box) as (x, y, w, l), and their IoU.  In the first two a 2 x 2 box
# lies inside a 4 x 2 box: the clip's crossing ratios d1 / (d1 - d2) are eighths, so every step is exact.  The third, two
# 3 x 1 boxes overlapping by 2 x 1, has crossing ratios 1/3 and 2/3, which round: its IoU is exactly 0.5 only because
# 3 * fl(1/3) and 3 * fl(2/3) round back to 1 and 2 in both precisions (tests/test_centerhead_edge_cases_cpu.py runs it).
IOU_PAIRS = [((4.5, 2.5, 4.0, 2.0), (5.0, 2.5, 2.0, 2.0), 0.5),
             ((5.0, 8.5, 2.0, 2.0), (4.5, 8.5, 4.0, 2.0), 0.5),
             ((3.5, 12.5, 3.0, 1.0), (4.5, 12.5, 3.0, 1.0), 0.5)]


# ------------------------------------------------------------------------------------------------------------ ties
def _ties_class(transposed):
    """5 x 7 (D0 != D1, 35 cells < 1024 threads: chunk 1), every cell at logit 0, K 10: cells 0..9 of the map AS HANDED.
    The velocity channel names the physical cell, so the transposed map's answer is a different set of boxes."""
    sc = Scene(5, 7, [1])
    for cell in range(35):
        sc.plant(cell, 0.0, vel=(cell, -cell))
    c = sc.case([[[(k, 0) for k in range(10)]]], max_num=10, coder_score_threshold=0.25, post_max_size=10)
    if transposed:
        c["h"] = np.ascontiguousarray(c["h"].transpose(0, 2, 1, 3))
        c["p"]["swapped"] = False
    return c


def _ties_kcut():
    """40 x 53 = 2120 cells (chunk 3, threads 707.. own nothing), K 64: 40 cells above the tied value, 100 AT it (0.5),
    30 below; neighbours are 2^-14 apart (key bit 10), so the first two radix passes cannot separate them and the third
    decides the cut.  The 24 smallest tied cells are taken."""
    sc = Scene(40, 53, [1])
    rng = np.random.default_rng(1)
    fixed = [0, 1, 2, 3, 5, 190, 191, 192, 193, 2117, 2118, 2119]      # one thread, two threads, two waves, the map's end
    rest = [int(c) for c in rng.permutation(2120) if c not in fixed]
    tied = sorted(fixed + rest[:88])
    hi, lo = rest[88:128], rest[128:158]
    for cell in tied:
        sc.plant(cell, 0.0)
    for k, cell in enumerate(hi, 1):
        sc.plant(cell, logit_of(0.5 + k * 2.0 ** -14))
    for k, cell in enumerate(lo, 1):
        sc.plant(cell, logit_of(0.5 - k * 2.0 ** -14))
    assert len(tied) == 100 and tied[23] // 3 // 64 >= 1                 # the taken ties span more than one wave
    expect = [(c, 0) for c in hi[::-1]] + [(c, 0) for c in tied[:24]]
    return sc.case([[expect]], max_num=64, coder_score_threshold=0.25, post_max_size=64)


def _ties_classes():
    """Task 0: 3 classes x K 8 = 24 candidates, padded to 32.  Task 1: 4 classes x 8 = 32, no padding.  Equal scores in
    several classes at the same and at different cells: class first, then cell; the K cut falls inside the ties."""
    sc = Scene(6, 5, [3, 4])
    for cls, cell, k in ((2, 9, 3), (1, 10, 2), (0, 11, 1), (0, 17, 0), (0, 4, 0), (2, 4, 0), (2, 3, 0), (1, 3, 0), (1, 29, 0),
                         (0, 20, -1), (2, 21, -2), (1, 22, -3)):
        sc.plant(cell, logit_k(k), t=0, cls=cls)
    e0 = [(9, 2), (10, 1), (11, 0), (4, 0), (17, 0), (3, 1), (29, 1), (3, 2)]             # (4, 2) and the lower three are cut
    for cls, cell, k in ((2, 5, 2), (3, 6, 1), (3, 7, 0), (1, 7, 0), (0, 12, 0), (3, 2, 0), (1, 2, 0), (0, 1, -1), (1, 0, -2)):
        sc.plant(cell, logit_k(k), t=1, cls=cls)
    e1 = [(5, 2), (6, 3), (12, 0), (2, 1), (7, 1), (2, 3), (7, 3), (1, 0)]
    return sc.case([[e0, e1]], coder_score_threshold=0.25, min_radius=[-1.0, -1.0])


# ------------------------------------------------------------------------------------------------------ thresholds
def _thresholds(kind):
    """Scores 0.731 (cell 6), exactly 0.5 (cell 5) and 0.269 (cell 9); the fourth candidate is background cell 0."""
    sc = Scene(4, 4, [1])
    sc.plant(6, 1.0)
    sc.plant(5, 0.0)
    sc.plant(9, -1.0)
    over, expect = {
        "coder_on": (dict(coder_score_threshold=0.5), [6]),                                # strict: 0.5 > 0.5 is false
        "coder_below": (dict(coder_score_threshold=below(0.5)), [6, 5]),
        "test_on": (dict(nms_type="rotate", coder_score_threshold=0.125, score_threshold=0.5), [6, 5]),      # closed
        "test_above": (dict(nms_type="rotate", coder_score_threshold=0.125, score_threshold=above(0.5)), [6]),
        "test_circle": (dict(coder_score_threshold=0.125, score_threshold=0.5), [6, 5, 9]),    # not applied on this path
        "falsy_none": (dict(coder_score_threshold=None, score_threshold=0.0), [6, 5, 9, 0]),
        "falsy_zero": (dict(nms_type="rotate", coder_score_threshold=0, score_threshold=0), [6, 5, 9, 0]),
    }[kind]
    return sc.case([[[(c, 0) for c in expect]]], max_num=4, **over)


# ---------------------------------------------------------------------------------------------------------- ranges
RANGE = [-2.5, -1.75, -1.0, 2.25, 3.5, 2.0]
STEP = 2.0 ** -10


def _ranges(kind):
    """8 x 8, pc_range (-4, -4): six objects, each with one coordinate exactly on one bound of RANGE, and one inside.
    x = ix + reg0 - 4, y = iy + reg1 - 4; the filters read the raw height, not the merged z."""
    sc = Scene(8, 8, [1])
    s = STEP if kind == "coder_step" else 0.0
    plants = [(1, 4, (0.5 - s, 0.5), 0.0), (3, 2, (0.5, 0.25 - s), 0.0), (4, 4, (0.5, 0.5), -1.0 - s),
              (6, 3, (0.25 + s, 0.5), 0.0), (2, 7, (0.5, 0.5 + s), 0.0), (5, 5, (0.5, 0.5), 2.0 + s), (3, 5, (0.5, 0.5), 0.0)]
    cells = [sc.plant(sc.cell(ix, iy), logit_k(7 - k), reg=reg, z=z) for k, (ix, iy, reg, z) in enumerate(plants)]
    tight = [above(v) for v in RANGE[:3]] + [below(v) for v in RANGE[3:]]
    over, expect = {
        "coder_on": (dict(post_center_range=RANGE), cells),
        "coder_ulp": (dict(post_center_range=tight), cells[6:]),
        "coder_step": (dict(post_center_range=RANGE), cells[6:]),
        "coder_on_rotate": (dict(post_center_range=RANGE, nms_type="rotate"), cells),
        "limit_on": (dict(post_center_limit_range=RANGE, nms_type="rotate"), cells),
        "limit_ulp": (dict(post_center_limit_range=tight, nms_type="rotate"), cells[6:]),
        "limit_circle": (dict(post_center_limit_range=tight), cells),                    # the circle path has no limit range
        "limit_none": (dict(post_center_limit_range=None, nms_type="rotate", post_center_range=tight), cells[6:]),
        "limit_empty": (dict(post_center_limit_range=[], nms_type="rotate"), cells),
    }[kind]
    return sc.case([[[(c, 0) for c in expect]]], pc_range=[-4.0, -4.0], **over)


def _limit_after_nms(limited):
    """A (4 x 4, best score) lies outside the limit range in y; B (4 x 4, 0.75 m further, inside) has IoU 13/19 with A
    and is suppressed BEFORE A is dropped; C is far away.  Without a limit range A stays."""
    sc = Scene(12, 12, [1])
    a = sc.plant(sc.cell(5, 1), logit_k(3), dim=(4, 4, 1))                    # y = 1.5 - 4 = -2.5 < -1.75
    sc.plant(sc.cell(5, 2), logit_k(2), reg=(0.5, 0.25), dim=(4, 4, 1))       # y = -1.75: on the bound, kept by the range
    c = sc.plant(sc.cell(5, 7), logit_k(1))
    expect = [c] if limited else [a, c]
    return sc.case([[[(k, 0) for k in expect]]], pc_range=[-4.0, -4.0], nms_type="rotate",
                   post_center_limit_range=RANGE if limited else None)


# ------------------------------------------------------------------------------------------------------------- NMS
def _circle(kind):
    sc = Scene(8, 8, [1])
    if kind == "chain":                           # A suppresses B (d2 4 <= 4); B would have suppressed C; A - C is 16
        cells = [sc.plant(sc.cell(ix, 1), logit_k(3 - k)) for k, ix in enumerate((1, 3, 5))]
        return sc.case([[[(cells[0], 0), (cells[2], 0)]]], min_radius=[4.0])
    p, q = sc.plant(sc.cell(1, 1), logit_k(2)), sc.plant(sc.cell(4, 5), logit_k(1))      # 3-4-5: d2 = 25
    if kind == "on":
        return sc.case([[[(p, 0)]]], min_radius=[25.0])
    return sc.case([[[(p, 0), (q, 0)]]], min_radius=[below(25.0)])


def _plant_box(sc, k, x, y, w, l, cls=0, t=0):
    """A box with centre (x, y) (pc_range 0): the cell of floor(x), floor(y) and the binary-fraction offset."""
    ix, iy = int(np.floor(x)), int(np.floor(y))
    return sc.plant(sc.cell(ix, iy), logit_k(k), t=t, cls=cls, reg=(x - ix, y - iy), dim=(w, l, 1))


def _rotate(kind):
    sc = Scene(16, 16, [1])
    if kind == "chain":                           # 2 x 2 boxes 0.5 m apart: IoU 3/5; A - C 1 m apart: IoU 1/3
        a = _plant_box(sc, 3, 2.5, 4.5, 2, 2)
        _plant_box(sc, 2, 3.0, 4.5, 2, 2)
        c = sc.plant(sc.cell(4, 4), logit_k(1), reg=(-0.5, 0.5), dim=(2, 2, 1))          # x = 3.5 from the next cell
        return sc.case([[[(a, 0), (c, 0)]]], nms_type="rotate")
    first, later = [], []
    for n, (a, b, _) in enumerate(IOU_PAIRS):
        first.append(_plant_box(sc, 12 - 2 * n, *a))
        later.append(_plant_box(sc, 11 - 2 * n, *b))
    if kind == "iou_on":                          # strict: IoU == nms_thr is kept
        expect = [c for pair in zip(first, later) for c in pair]
        return sc.case([[[(c, 0) for c in expect]]], nms_type="rotate", nms_thr=0.5)
    return sc.case([[[(c, 0) for c in first]]], nms_type="rotate", nms_thr=below(0.5))


def _identical_and_zero_area():
    """Two classes in one cell share the cell's geometry: identical 2 x 2 boxes (IoU 1: the later one goes), and identical
    0 x 0 boxes (intersection 0 over max(0, 1e-8): IoU 0, both stay)."""
    sc = Scene(8, 8, [2])
    x = sc.cell(2, 2)
    sc.plant(x, logit_k(4), cls=1, dim=(2, 2, 1))
    sc.plant(x, logit_k(3), cls=0)
    y = sc.cell(5, 5)
    sc.plant(y, logit_k(2), cls=0, dim=(0, 0, 1))
    sc.plant(y, logit_k(1), cls=1)
    return sc.case([[[(x, 1), (y, 0), (y, 1)]]], nms_type="rotate")


def _nms_scale():
    """2 x 2 boxes 2.5 m apart do not overlap.  Class 0 is scaled by 2: 4 x 4 boxes, IoU 6/26 > 1/8; class 1 is not."""
    sc = Scene(16, 16, [2])
    a = _plant_box(sc, 4, 2.5, 2.5, 2, 2, cls=0)
    _plant_box(sc, 3, 5.0, 2.5, 2, 2, cls=0)
    c = _plant_box(sc, 2, 2.5, 10.5, 2, 2, cls=1)
    d = _plant_box(sc, 1, 5.0, 10.5, 2, 2, cls=1)
    return sc.case([[[(a, 0), (c, 1), (d, 1)]]], nms_type="rotate", nms_thr=0.125, nms_scale=[[2.0, 1.0]])


def _pre_max(kind):
    """Six survivors; the second overlaps the first (identical centre offset 0.5: IoU 3/5).  pre_max 4 cuts BEFORE the
    NMS: ranks 0, 2, 3 come out, and rank 4, which nothing would suppress, does not.  The circle path has no pre_max."""
    sc = Scene(16, 16, [1])
    cells = [_plant_box(sc, 6, 2.5, 2.5, 2, 2), _plant_box(sc, 5, 3.0, 2.5, 2, 2)]
    cells += [_plant_box(sc, 4 - k, 2.5 + 4 * (k % 2), 7.5 + 3 * (k // 2), 2, 2) for k in range(4)]
    if kind == "rotate":
        return sc.case([[[(cells[k], 0) for k in (0, 2, 3)]]], nms_type="rotate", pre_max_size=4)
    return sc.case([[[(c, 0) for c in cells]]], pre_max_size=4)


def _post_max(post, kind):
    """Twelve survivors, none suppressing another: the first ``post`` come out."""
    sc = Scene(8, 8, [1])
    cells = [sc.plant((k * 11) % 64, logit_k(12 - k)) for k in range(12)]
    return sc.case([[[(c, 0) for c in cells[:post]]]], max_num=16, nms_type=kind, post_max_size=post)


# ----------------------------------------------------------------------------------------------------------- sizes
def _ranked(D0, D1, ncls, K, post, seed):
    """Every (class, cell) gets its own logit k * 2^-12, k a permutation: the top ``post`` of all of them come out."""
    sc = Scene(D0, D1, [ncls])
    hw = D0 * D1
    ks = np.random.default_rng(seed).permutation(ncls * hw)
    for flat, k in enumerate(ks):
        sc.plant(flat % hw, logit_k(int(k)), cls=flat // hw)
    order = np.argsort(-ks, kind="stable")[:post]
    return sc.case([[[(int(f) % hw, int(f) // hw) for f in order]]], max_num=K, post_max_size=post, coder_score_threshold=None,
                   min_radius=[-1.0])


def _all_cells_tied():
    """32 x 32, max_num == D0 * D1: every cell is a candidate, all at 0.5: cells 0..511."""
    sc = Scene(32, 32, [1])
    for cell in range(1024):
        sc.plant(cell, 0.0)
    return sc.case([[[(k, 0) for k in range(512)]]], max_num=1024, post_max_size=512)


def _k1():
    """max_num 1: N = 2 entries to sort.  Task 0: class 1 is better.  Task 1: a tie: class 0 wins over the smaller cell."""
    sc = Scene(3, 3, [2, 2])
    sc.plant(4, logit_k(1), t=0, cls=0)
    sc.plant(2, logit_k(2), t=0, cls=1)
    sc.plant(0, 0.0, t=1, cls=1)
    sc.plant(8, 0.0, t=1, cls=0)
    return sc.case([[[(2, 1)], [(8, 0)]]], max_num=1, post_max_size=1)


TASKS8 = [1, 2, 1, 3, 1, 4, 2, 1]


def _tasks8():
    """Eight tasks, two samples, both NMS kinds, label offsets up to 14.  Task 3's objects all fail the score filter and
    task 6's the centre range: count 0."""
    sc = Scene(6, 7, TASKS8, B=2)
    expect = [[], []]
    for b in range(2):
        for t, ncls in enumerate(TASKS8):
            got = []
            for j in range(3):
                cell = (t * 3 + b * 5 + j * 9) % 42
                sc.plant(cell, -8.0 if t == 3 else logit_k(3 - j), t=t, cls=j % ncls, b=b, z=100.0 if t == 6 else float(j))
                got.append((cell, j % ncls))
            expect[b].append([] if t in (3, 6) else got)
    return sc.case(expect, max_num=4, post_max_size=4, nms_type=["circle", "rotate"] * 4)


# ------------------------------------------------------------------------------------------------------ non-finite
def _nan_heat(kind):
    """No score filter, K 8, three objects: five background cells (score 0, smallest cells first) fill the candidates.
    ``h_nan`` has NaN instead of -inf in cells 0, 2, 5 and 19: the key rule NaN -> 0 must rank them as background.
    (The reference's torch.topk would rank NaN first: this pins the device rule, not the reference's.)"""
    sc = Scene(4, 5, [1])
    for k, cell in enumerate((7, 11, 13)):
        sc.plant(cell, logit_k(3 - k))
    c = sc.case([[[(7, 0), (11, 0), (13, 0)] + [(k, 0) for k in range(5)]]], nms_type=kind, coder_score_threshold=None)
    c["h_nan"] = c["h"].copy()
    heat = sc.chan[0][0]
    for cell in (0, 2, 5, 19):
        c["h_nan"].reshape(1, 20, -1)[0, cell, heat] = np.nan
    return c


def _posinf():
    sc = Scene(4, 4, [1])
    sc.plant(3, 5.0)
    sc.plant(9, np.inf)                           # exactly 1.0, first
    sc.plant(12, 0.0)
    return sc.case([[[(9, 0), (3, 0), (12, 0)]]], nms_type="rotate")


def _nan_geometry():
    """The three best objects have a NaN centre x, a NaN centre y and a NaN height: the closed range filter drops them
    (every comparison with NaN is false) before the NMS; the two others come out undisturbed."""
    sc = Scene(6, 6, [1])
    sc.plant(7, logit_k(5), reg=(np.nan, 0.5))
    sc.plant(8, logit_k(4), reg=(0.5, np.nan))
    sc.plant(14, logit_k(3), z=np.nan)
    sc.plant(15, logit_k(2))
    sc.plant(20, logit_k(1))
    return sc.case([[[(15, 0), (20, 0)]]], nms_type="rotate")


BUILDERS = {
    "ties_class_5x7_swapped": lambda: _ties_class(False),
    "ties_class_7x5_reference": lambda: _ties_class(True),
    "ties_kcut_40x53": _ties_kcut,
    "ties_classes_3_and_4": _ties_classes,
    **{f"thr_{k}": functools.partial(_thresholds, k)
       for k in ("coder_on", "coder_below", "test_on", "test_above", "test_circle", "falsy_none", "falsy_zero")},
    **{f"range_{k}": functools.partial(_ranges, k)
       for k in ("coder_on", "coder_ulp", "coder_step", "coder_on_rotate", "limit_on", "limit_ulp", "limit_circle", "limit_none",
                 "limit_empty")},
    "limit_after_nms": lambda: _limit_after_nms(True),
    "limit_after_nms_none": lambda: _limit_after_nms(False),
    **{f"circle_{k}": functools.partial(_circle, k) for k in ("on", "below", "chain")},
    **{f"rotate_{k}": functools.partial(_rotate, k) for k in ("iou_on", "iou_below", "chain")},
    "rotate_identical_and_zero_area": _identical_and_zero_area,
    "rotate_nms_scale": _nms_scale,
    "pre_max_rotate": lambda: _pre_max("rotate"),
    "pre_max_circle": lambda: _pre_max("circle"),
    "post_max_8_circle": lambda: _post_max(8, "circle"),
    "post_max_8_rotate": lambda: _post_max(8, "rotate"),
    "post_max_1": lambda: _post_max(1, "rotate"),
    "post_max_512_of_600": lambda: _ranked(32, 32, 1, 600, 512, 3),
    "maxcand_2x1024": lambda: _ranked(32, 32, 2, 1024, 512, 4),          # CT_MAXK, CT_MAXCAND and max_num == D0 * D1
    "k512_4_classes": lambda: _ranked(23, 29, 4, 512, 512, 5),           # CT_MAXCLS at CT_MAXCAND
    "all_cells_tied_32x32": _all_cells_tied,
    "k1_two_tasks": _k1,
    "tasks_8_b2": _tasks8,
    "nan_heat_circle": lambda: _nan_heat("circle"),
    "nan_heat_rotate": lambda: _nan_heat("rotate"),
    "posinf_first": _posinf,
    "nan_geometry": _nan_geometry,
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def refusal_scene():
    """A 33 x 32 map (1056 cells, so that max_num 1025 passes the cell count) for the refusals."""
    sc = Scene(33, 32, [1])
    sc.plant(5, 0.0)
    return sc
