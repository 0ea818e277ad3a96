"""Generated inputs for the box-wise IoU estimator (csrc/estimator.hip), shared by the GPU test
(tests/test_estimator_edges_gpu.py) and the CPU checks of the cases themselves (tests/test_estimator_cases_cpu.py).
Imports numpy and the float64 yardstick tests/estimator_numpy.py only; every case comes from a fixed seed.

``case(name)`` -> dict(boxes [B,nt,post,D] f32, labels [B,nt,post] i32, counts [B,nt] i32, points [P,F] f32, offsets
[B+1] i64, num_classes, rot_col, classes (the class count of every task of the module whose weights the case is run
with), dropped (the share of points the margin rule took), exempt (indices of the points written after the margin rule),
hits, reach).  ``hits[b]`` = (slots, mask): the frame's valid slots ``t * post + i`` in the kernel's task-major order and
``EN.inside`` of every point of the frame for each of them.  ``reach`` holds the properties a case exists for, computed
from ``hits`` on the final points, never assumed:

  frames_hit      frames in which some box holds a point
  tiles           wave tiles (EST_WTILE points) per frame
  levels          {(frame, tile): the wave's queue level after each valid box}, by the kernel's rule: a box appends its
                  hits in the tile, and the queue is drained when it then stands above EST_QCAP - EST_WTILE
  drains          {(frame, tile): mid-loop drains} (the final drain not counted)
  survivors       {(frame, task): slots that hold a point, ascending}
  two_tile_boxes  (frame, slot) of the boxes with hits in more than one tile
plus what the families add (see the builders).

THE MARGIN RULE, as tools/gen_golden_estimator.py enforces it for the golden fixture: membership is a strict inequality
on float32 products, so a point within 1e-3 m of an edge of a doubled footprint (``EN.edge_distance`` on
``EN.footprint``), or with ||pz - z| - h/2| < 1e-3 m, may legitimately fall either way.  Every such point, for any
finite box within its frame's counts, is dropped: moved to a spot of its own beyond (250, 250) m, which keeps the frame's
point count and every other point's index (a wave tile is a range of indices).  More than 5 % dropped raises.  Written
AFTER the rule and exempt from it (``exempt``): the exact-boundary points of the values family, which are exact in both
precisions by construction, and its NaN / inf points, which have no distance to anything.

Families: ``A`` frames, ``B1`` / ``B2`` queue, ``C`` many boxes, ``D`` cap, ``E_*`` layouts, ``F_*`` values."""
import functools

import numpy as np

import estimator_numpy as EN

# Mirrors of csrc/estimator.hip's defines and of AL3D_EST_MAX_BOXES (include/al3d.h).  The reach assertions of
# tests/test_estimator_cases_cpu.py are stated in these numbers: a kernel whose constants move must fail them.
T = 512                 # EST_WTILE = 64 * EST_PPL: points per wave
Q = 1024                # EST_QCAP: queue entries per wave
WAVES = 4               # EST_WAVES: waves per workgroup of the points and head kernels
GROUP = 4               # EST_GROUP: boxes per wave pass of the head
CHUNK = 64              # boxes per trip of the ballot compactions (one per lane)
MAX_BOXES = 1024        # AL3D_EST_MAX_BOXES: nt * post

MARGIN = 1e-3
MAX_DROPPED = 0.05
DEFAULT_CLASSES = (4, 6)
NAMES = ("A", "B1", "B2", "C", "D", "E_dim7", "E_dim11_rot8", "E_f3", "E_f6", "E_nc3", "E_nc32", "E_tail",
         "F_clean", "F_dirty1", "F_dirty2", "F_counts")


# ------------------------------------------------------------------------------------------------------------ pieces
def _grid(n, cell):
    """Centres of at least ``n`` square cells of ``cell`` metres, centred on the origin."""
    k = int(np.ceil(np.sqrt(n)))
    c = (np.arange(k) - (k - 1) / 2) * cell
    return [(float(x), float(y)) for x in c for y in c]


def _box(rng, cx, cy, D, rot_col, wl=((0.6, 2.5), (0.8, 4.5)), jitter=2.0):
    """A random box row around (cx, cy): sizes from ``wl``, angle in +-7 rad at ``rot_col``, junk in the other columns."""
    row = rng.normal(size=D) * 3.0
    row[:6] = [cx + rng.uniform(-jitter, jitter), cy + rng.uniform(-jitter, jitter), rng.uniform(-1, 1),
               rng.uniform(*wl[0]), rng.uniform(*wl[1]), rng.uniform(1.0, 3.0)]
    row[rot_col] = rng.uniform(-7.0, 7.0)
    return row.astype(np.float32)


def _world(box, u, v, rot_col):
    """World xy of the footprint-local position (u, v): the polygon's sense of rotation (``EN.footprint``)."""
    c, s = np.cos(float(box[rot_col])), np.sin(float(box[rot_col]))
    return u * c + v * s + float(box[0]), -u * s + v * c + float(box[1])


def _cloud(rng, box, n, rot_col, above=False, spread=0.9, zband=(0.4, 0.55)):
    """``n`` points inside the doubled footprint, ``spread`` of its half extents at most; within ``zband[0]`` h of the
    centre's height, or (``above``) ``zband[1]`` .. 2 h above it: inside the footprint, outside the height."""
    u = rng.uniform(-spread, spread, n) * float(box[3])
    v = rng.uniform(-spread, spread, n) * float(box[4])
    x, y = _world(box, u, v, rot_col)
    dz = rng.uniform(zband[1], 2.0, n) if above else rng.uniform(-zband[0], zband[0], n)
    return np.stack([x, y, float(box[2]) + dz * float(box[5])], 1)


def _background(rng, n, extent):
    """Points above every box (the boxes' tops stay below 2.5 m)."""
    return np.stack([rng.uniform(-extent, extent, n), rng.uniform(-extent, extent, n), rng.uniform(6.0, 9.0, n)], 1)


def _frame(rng, boxes, rot_col, n_points, populate, above=(), last=None, extent=50.0, zband=(0.4, 0.55)):
    """One frame's xyz: ``populate`` {(t, i): n} clouds, ``above`` [(t, i)] boxes that get 6 points over their heads,
    background up to ``n_points``, shuffled; ``last`` = (t, i): that box's only point, at the frame's last index.
    -> (xyz [n_points, 3] f64, indices of the background points)."""
    parts = [_cloud(rng, boxes[t, i], n, rot_col, zband=zband) for (t, i), n in populate.items()]
    parts += [_cloud(rng, boxes[t, i], 6, rot_col, above=True, zband=zband) for t, i in above]
    fg = np.concatenate(parts) if parts else np.zeros((0, 3))
    tail = _cloud(rng, boxes[last], 1, rot_col, spread=0.5) if last is not None else np.zeros((0, 3))
    n_bg = n_points - len(fg) - len(tail)
    assert n_bg >= 0, "more planted points than the frame holds"
    body = np.concatenate([fg, _background(rng, n_bg, extent)])
    order = rng.permutation(len(body))
    is_bg = (np.arange(len(body)) >= len(fg))[order]
    return np.concatenate([body[order], tail]), np.nonzero(is_bg)[0]


# With hundreds of boxes in a frame the height half of the margin rule, which holds for a point wherever it lies in the
# plane, would take a tenth of the points and more.  The many-box cases therefore keep every box's z - h/2 and z + h/2 on
# multiples of 0.25 m (z on 0.25, h on 0.5) and every point's height 0.01 .. 0.24 m above such a multiple: none is dropped
# for its height.  A point moves by less than 0.25 m, which ``ZBAND_GRID`` leaves room for with h >= 1.
ZBAND_GRID = (0.2, 0.8)


def _planes_on_grid(boxes):
    boxes[..., 2] = np.round(boxes[..., 2] * 4) / 4
    boxes[..., 5] = np.round(boxes[..., 5] * 2) / 2
    return boxes


def _off_the_planes(rng, xyz):
    xyz[:, 2] = np.floor(xyz[:, 2] * 4) / 4 + rng.uniform(0.01, 0.24, len(xyz))
    return xyz


def _pack_points(rng, frames, F, tail_rows=0):
    """Frames back to back with ``F - 3`` extra columns; ``tail_rows`` rows behind the last offset repeat frame 0."""
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    xyz = np.concatenate(list(frames) + ([frames[0][:tail_rows]] if tail_rows else []))
    pts = np.concatenate([xyz, rng.uniform(0, 1, size=(len(xyz), F - 3))], 1).astype(np.float32)
    return pts, offsets


def _labels(rng, B, post, classes):
    """Labels of task t within its own classes, as the detector's heads emit them."""
    lo = np.concatenate([[0], np.cumsum(classes)])
    return np.stack([rng.integers(lo[t], lo[t + 1], size=(B, post)) for t in range(len(classes))], 1).astype(np.int32)


def _clamped(counts, post):
    return np.clip(np.asarray(counts, dtype=np.int64), 0, post)


def _finite(box, rot_col):
    return bool(np.isfinite(box[:6]).all() and np.isfinite(box[rot_col]))


def _enforce_margin(c, dropped=0):
    """The margin rule of the module docstring, in place on ``c['points']``; sets ``c['dropped']``.  ``dropped``: points
    an earlier pass over the same array has moved already (the values family shares one array among its variants)."""
    B, nt, post = c["labels"].shape
    cnt = _clamped(c["counts"], post)
    pts, off = c["points"], c["offsets"]
    for b in range(B):
        p = pts[off[b]:off[b + 1], :3].astype(np.float64)
        if not len(p):
            continue
        ok = np.ones(len(p), dtype=bool)
        for t in range(nt):
            for i in range(int(cnt[b, t])):
                box = c["boxes"][b, t, i]
                if not _finite(box, c["rot_col"]):
                    continue
                ok &= EN.edge_distance(p[:, :2], EN.footprint(box, c["rot_col"])) >= MARGIN
                ok &= np.abs(np.abs(p[:, 2] - float(box[2])) - float(box[5]) / 2) >= MARGIN
        for k in np.nonzero(~ok)[0]:
            pts[off[b] + k, :3] = [250.0 + 0.5 * dropped, 250.0 + 0.25 * b, 0.0]
            dropped += 1
    c["dropped"] = dropped / max(int(off[-1]), 1)
    if c["dropped"] > MAX_DROPPED:
        raise ValueError(f"{c['dropped']:.2%} of the points lie within {MARGIN} m of a membership boundary")
    return dropped


def _finish(c):
    """``hits`` and the common ``reach`` entries, from ``EN.inside`` on the final points."""
    B, nt, post = c["labels"].shape
    cnt = _clamped(c["counts"], post)
    pts, off = c["points"], c["offsets"]
    hits, levels, drains, survivors, two_tile, tiles = [], {}, {}, {}, [], []
    with np.errstate(invalid="ignore"):
        for b in range(B):
            p = pts[off[b]:off[b + 1]]
            slots = [t * post + i for t in range(nt) for i in range(int(cnt[b, t]))]
            mask = np.zeros((len(slots), len(p)), dtype=bool)
            if len(p):
                for k, s in enumerate(slots):
                    mask[k] = EN.inside(p, c["boxes"][b, s // post, s % post], c["rot_col"])
            hits.append((slots, mask))
            n_tiles = -(-len(p) // T)
            tiles.append(n_tiles)
            per_tile = np.stack([mask[:, w * T:(w + 1) * T].sum(1) for w in range(n_tiles)], 1) if n_tiles else \
                np.zeros((len(slots), 0), dtype=np.int64)
            for w in range(n_tiles):
                level, seen, n_drains = 0, [], 0
                for k in range(len(slots)):
                    level += int(per_tile[k, w])
                    seen.append(level)
                    if level > Q - T:
                        level, n_drains = 0, n_drains + 1
                levels[(b, w)], drains[(b, w)] = seen, n_drains
            two_tile += [(b, s) for k, s in enumerate(slots) if (per_tile[k] > 0).sum() > 1]
            for t in range(nt):
                survivors[(b, t)] = [s % post for k, s in enumerate(slots) if s // post == t and mask[k].any()]
    c["hits"] = hits
    c["reach"].update(frames_hit=[b for b in range(B) if hits[b][1].any()], tiles=tiles, levels=levels, drains=drains,
                      survivors=survivors, two_tile_boxes=two_tile)
    return c


def _case(boxes, labels, counts, points, offsets, classes=DEFAULT_CLASSES, rot_col=EN.ROT_COL, **reach):
    return dict(boxes=np.ascontiguousarray(boxes, dtype=np.float32), labels=np.ascontiguousarray(labels, dtype=np.int32),
                counts=np.asarray(counts, dtype=np.int32), points=points, offsets=offsets, classes=tuple(classes),
                num_classes=int(sum(classes)), rot_col=rot_col, exempt=[], reach=dict(reach))


# ------------------------------------------------------------------------------------------------------- A and its kin
# frame 0 of A (and all of F): task 0 slots 0..4 and task 1 slots 0..5 hold points; (1, 6) and (0, 5..7) hold none, the
# values family rewrites (0, 5..7) and (1, 7)
_A_POPULATED = [(0, i) for i in range(5)] + [(1, i) for i in range(6)]


def _boxes_on_grid(rng, B, nt, post, D, rot_col, cell=20.0):
    cells = _grid(nt * post, cell)
    boxes = np.zeros((B, nt, post, D), dtype=np.float32)
    for b in range(B):
        order = rng.permutation(len(cells))
        for t in range(nt):
            for i in range(post):
                boxes[b, t, i] = _box(rng, *cells[order[t * post + i]], D, rot_col)
    return boxes


def _build_a():
    """A: four frames of 700 / 0 / 513 / 40 points = 2 + 0 + 2 + 1 wave tiles over two workgroups.  Frame 2 starts at
    wave 2 of workgroup 0 and its second tile is one point, the only point of its box (1, 2).  Frame 1 has valid boxes
    and no point; slots behind the counts of frames 2 and 3 have points around them and must stay at 0."""
    rng = np.random.default_rng(101)
    boxes = _boxes_on_grid(rng, 4, 2, 8, 9, 6)
    counts = [[8, 8], [8, 5], [6, 8], [8, 3]]
    f0, _ = _frame(rng, boxes[0], 6, 700, {s: int(rng.integers(20, 45)) for s in _A_POPULATED}, above=[(1, 6)])
    f2, _ = _frame(rng, boxes[2], 6, 513, {(0, 0): 40, (0, 2): 35, (0, 5): 30, (1, 0): 45, (1, 4): 25, (0, 7): 30},
                   above=[(0, 3)], last=(1, 2))
    f3, _ = _frame(rng, boxes[3], 6, 40, {(0, 1): 8, (0, 6): 7, (1, 1): 9, (1, 5): 6})
    pts, off = _pack_points(rng, [f0, np.zeros((0, 3)), f2, f3], 5)
    c = _case(boxes, _labels(rng, 4, 8, DEFAULT_CLASSES), counts, pts, off, lone_tile=(2, 1), lone_box=(2, 1 * 8 + 2))
    _enforce_margin(c)
    return _finish(c)


def _build_layout(seed, D=9, rot_col=6, F=5, classes=DEFAULT_CLASSES, tail_rows=0):
    """E: two frames of 530 / 90 points (2 + 1 wave tiles), post 8, one task per entry of ``classes``; every frame has
    boxes with points, boxes without, and points over a box's head."""
    rng = np.random.default_rng(seed)
    nt = len(classes)
    boxes = _boxes_on_grid(rng, 2, nt, 8, D, rot_col)
    slots = [(t, i) for t in range(nt) for i in range(8)]
    empty0, empty1 = {(0, 3), (nt - 1, 6)}, {(0, 0), (nt - 1, 7)}
    per0 = 300 // (len(slots) - 2)
    f0, _ = _frame(rng, boxes[0], rot_col, 530, {s: int(rng.integers(per0 - 6, per0 + 6)) for s in slots if s not in empty0},
                   above=sorted(empty0))
    f1, _ = _frame(rng, boxes[1], rot_col, 90, {s: int(rng.integers(2, 5)) for s in slots if s not in empty1 and s[1] < 7},
                   above=[(0, 0)])
    pts, off = _pack_points(rng, [f0, f1], F, tail_rows)
    counts = np.full((2, nt), 8)
    counts[1, 0] = 7                                        # (1, 0, 7) sits behind the count, with points around it
    labels = _labels(rng, 2, 8, classes)
    labels[0, 0, 0], labels[0, nt - 1, 1] = 0, sum(classes) - 1       # the first and the last one-hot column are used
    c = _case(boxes, labels, counts, pts, off, classes=classes, rot_col=rot_col, tail_rows=tail_rows)
    _enforce_margin(c)
    return _finish(c)


# ---------------------------------------------------------------------------------------------------------------- B
def _queue_points(rng):
    n = 2 * T + 37
    xyz = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-1, 1, n)], 1)
    return _pack_points(rng, [xyz], 5)


def _all_point_box(rng, D=9):
    """Doubled footprint 120 m x 120 m at any angle around a centre inside the points' square: holds all of it."""
    row = _box(rng, 0.0, 0.0, D, 6, wl=((58.0, 62.0), (58.0, 62.0)), jitter=5.0)
    row[2], row[5] = 0.0, 8.0
    return row


def _build_b1():
    """B1: one frame of 2 T + 37 points; boxes 0, 1 and 3 hold every point, box 2 the half with x in (0, 20).  A full
    tile queues 512, then 1024 = EST_QCAP exactly (queue index 1023; drain), then about 250, then 512 more (drain); the
    37-point tile only sees the final drain."""
    rng = np.random.default_rng(202)
    pts, off = _queue_points(rng)
    boxes = np.stack([_all_point_box(rng), _all_point_box(rng), _all_point_box(rng), _all_point_box(rng)])
    boxes[2, :7] = [10.0, 0.0, 0.0, 10.0, 60.0, 8.0, 0.0]
    labels = np.array([[[1, 9, 4, 0]]])
    c = _case(boxes[None, None], labels, [[4]], pts, off)
    _enforce_margin(c)
    return _finish(c)


def _build_b2():
    """B2: the points of B1; box 0 holds exactly one point (index 5, in tile 0), boxes 1 and 2 hold every point, slot 3
    is behind the count.  Tile 0 queues 1, then 513 = EST_QCAP - EST_WTILE + 1 (drain), then 512 (final drain)."""
    rng = np.random.default_rng(202)
    pts, off = _queue_points(rng)
    boxes = np.stack([_all_point_box(rng), _all_point_box(rng), _all_point_box(rng), _all_point_box(rng)])
    boxes[0, :7] = [pts[5, 0], pts[5, 1], 0.0, 0.05, 0.05, 8.0, 0.7]       # 0.1 m x 0.1 m around the point, any height
    labels = np.array([[[7, 2, 5, 3]]])
    c = _case(boxes[None, None], labels, [[3]], pts, off, lone_point=5)
    _enforce_margin(c)
    return _finish(c)


# ---------------------------------------------------------------------------------------------------------------- C
C_COUNTS = [[160, 70], [65, 0]]


def _build_c():
    """C: post 160, counts [[160, 70], [65, 0]].  Every slot, valid or not, is a box of 0.5 .. 2.5 m in an 8 m cell of
    its own with 1 .. 6 points; valid slots i with i % 5 == 3 are left empty (63, 68, 128, 133, ... among them), and so
    are the first 1 / 2 / 3 other slots of (0, 0) / (0, 1) / (1, 0), which leaves 127 / 54 / 49 survivors: residues 3, 2
    and 1 mod EST_GROUP.  Every third empty box has points over its head.  (1, 1) has count 0: nothing survives there."""
    rng = np.random.default_rng(303)
    B, nt, post = 2, 2, 160
    cells = _grid(nt * post, 8.0)
    boxes = np.zeros((B, nt, post, 9), dtype=np.float32)
    frames = []
    extra = {(0, 0): 1, (0, 1): 2, (1, 0): 3}
    for b in range(B):
        order = rng.permutation(len(cells))
        populate, above = {}, []
        for t in range(nt):
            left = extra.get((b, t), 0)
            for i in range(post):
                boxes[b, t, i] = _planes_on_grid(_box(rng, *cells[order[t * post + i]], 9, 6, wl=((0.5, 2.5), (0.5, 2.5)),
                                                      jitter=0.4))
                valid = i < C_COUNTS[b][t]
                if valid and i % 5 == 3:
                    if (i // 5) % 3 == 0:
                        above.append((t, i))
                elif valid and left:
                    left -= 1
                else:
                    populate[(t, i)] = int(rng.integers(1, 7))
        n = sum(populate.values()) + 6 * len(above)
        frames.append(_off_the_planes(rng, _frame(rng, boxes[b], 6, n + 60, populate, above=above, extent=75.0,
                                                  zband=ZBAND_GRID)[0]))
    pts, off = _pack_points(rng, frames, 5)
    c = _case(boxes, _labels(rng, B, post, DEFAULT_CLASSES), C_COUNTS, pts, off)
    _enforce_margin(c)
    return _finish(c)


# ---------------------------------------------------------------------------------------------------------------- D
def _build_d():
    """D: one task of AL3D_EST_MAX_BOXES = 1024 valid boxes on a 32 x 32 grid of 6 m cells, 1 .. 4 points each and no
    other point: every box survives, ``s_list`` is full, the queue's box index runs to 1023."""
    rng = np.random.default_rng(404)
    cells = _grid(MAX_BOXES, 6.0)
    order = rng.permutation(len(cells))
    boxes = _planes_on_grid(np.stack([_box(rng, *cells[order[i]], 9, 6, wl=((0.5, 1.8), (0.5, 1.8)), jitter=0.4)
                                      for i in range(MAX_BOXES)]))
    xyz = np.concatenate([_cloud(rng, boxes[i], int(rng.integers(1, 5)), 6, spread=0.8, zband=ZBAND_GRID)
                          for i in range(MAX_BOXES)])
    xyz = _off_the_planes(rng, xyz[rng.permutation(len(xyz))])
    pts, off = _pack_points(rng, [xyz], 5)
    c = _case(boxes[None, None], rng.integers(0, 10, size=(1, 1, MAX_BOXES)), [[MAX_BOXES]], pts, off)
    _enforce_margin(c)
    return _finish(c)


# ---------------------------------------------------------------------------------------------------------------- F
EDGE_BOX = np.float32([64.0, 4.0, 0.5, 1.0, 2.0, 2.0, 0.0, 0.25, -0.5])     # dyadic, angle 0: footprint [63, 65] x [2, 6]
EDGE_POINTS = [                                                             # (xyz, inside)
    ((64.0, 4.0, 1.5), True),                                               # z + h / 2 exactly: the height test is inclusive
    ((64.0, 4.0, float(np.nextafter(np.float32(1.5), np.float32(2)))), False),
    ((64.0, 4.0, -0.5), True),                                              # z - h / 2 exactly
    ((65.0, 4.0, 0.5), False),                                              # on the footprint's edge: the test is strict
    ((float(np.nextafter(np.float32(65), np.float32(0))), 4.0, 0.5), True),  # one f32 ulp inside that edge
    ((64.0, 2.0, 0.5), False),                                              # on the edge along y
    ((64.0, float(np.nextafter(np.float32(2), np.float32(3))), 0.5), True),
]
F_DIRTY_SLOTS = [(0, 5), (0, 6), (0, 7)]


F_VARIANTS = ("clean", "dirty1", "dirty2", "counts")


def _f_boxes(clean, variant):
    """-> (boxes, bad points) of a variant: slots (0, 5..7) of the clean table rewritten."""
    boxes = clean.copy()
    base = clean[0, 0, 0].copy()
    x, y, z = (float(v) for v in base[:3])
    if variant == "dirty1":
        boxes[0, 0, 5:8] = base
        boxes[0, 0, 5, 0] = np.nan
        boxes[0, 0, 6, 6] = np.nan
        boxes[0, 0, 7, 3] = 0.0
        return boxes, [(np.nan, y, z), (np.inf, y, z), (x, y, -np.inf)]
    if variant == "dirty2":
        boxes[0, 0, 5:8] = base
        boxes[0, 0, 5, 3] = -1.5
        boxes[0, 0, 6, 3] = np.nan
        boxes[0, 0, 7, 5] = -1.0
        return boxes, [(-np.inf, y, z), (x, np.nan, z)]
    return boxes, []


@functools.lru_cache(maxsize=None)
def _build_f():
    """F: frame 0 of A's layout (same seed, so the same boxes and clouds) as a batch of one, with the exact-boundary box
    ``EDGE_BOX`` at (1, 7) and ``EDGE_POINTS`` written over background points.  Slots (0, 5..7):

      clean   ordinary boxes 300 m and more from every point
      dirty1  a NaN centre; a NaN angle; w = 0 -- otherwise copies of the populated box (0, 0), so they sit on top of
              it; three background points become (NaN, y, z), (inf, y, z), (x, y, -inf), with x, y, z the centre of (0, 0)
      dirty2  w = -1.5; w = NaN (the reject radius is NaN); h = -1 -- otherwise copies of (0, 0); two background points
              become (-inf, y, z) and (x, NaN, z)
      counts  the clean boxes with counts [post + 5, -3]: the kernel clamps them to [post, 0]

    The margin rule runs over ONE point array for the finite boxes of every variant, so the variants' points differ in
    the rewritten background points alone, and every slot that is ordinary in two variants holds the same points in
    both.  -> {variant: case}"""
    rng = np.random.default_rng(101)
    clean = _boxes_on_grid(rng, 4, 2, 8, 9, 6)[:1].copy()
    f0, bg = _frame(rng, clean[0], 6, 700, {s: int(rng.integers(20, 45)) for s in _A_POPULATED}, above=[(1, 6)])
    rng = np.random.default_rng(606)
    pts, off = _pack_points(rng, [f0], 5)
    labels = _labels(rng, 1, 8, DEFAULT_CLASSES)
    clean[0, 1, 7] = EDGE_BOX
    for k, (t, i) in enumerate(F_DIRTY_SLOTS):
        clean[0, t, i, 0] = -300.0 - 20.0 * k
    cases, dropped = {}, 0
    for variant in F_VARIANTS:
        boxes, bad = _f_boxes(clean, variant)
        c = _case(boxes, labels, [[8 + 5, -3]] if variant == "counts" else [[8, 8]], pts, off, edge_slot=1 * 8 + 7,
                  dirty_slots=[t * 8 + i for t, i in F_DIRTY_SLOTS])
        dropped = _enforce_margin(c, dropped)
        cases[variant] = (c, bad)
    # after the rule, over background points (6 .. 9 m up: inside no box), at the same indices in every variant
    spots = [int(k) for k in bg[:len(EDGE_POINTS) + 3]]
    out = {}
    for variant, (c, bad) in cases.items():
        c["points"] = pts.copy()
        c["dropped"] = dropped / len(pts)
        for k, (xyz, _) in zip(spots, EDGE_POINTS):
            c["points"][k, :3] = xyz
        for k, xyz in zip(spots[len(EDGE_POINTS):], bad):
            c["points"][k, :3] = xyz
        c["exempt"] = spots[:len(EDGE_POINTS) + len(bad)]
        c["reach"].update(edge_points=spots[:len(EDGE_POINTS)], bad_points=spots[len(EDGE_POINTS):][:len(bad)])
        out[variant] = _finish(c)
    return out


_BUILDERS = {
    "A": _build_a, "B1": _build_b1, "B2": _build_b2, "C": _build_c, "D": _build_d,
    "E_dim7": lambda: _build_layout(501, D=7, rot_col=6),
    "E_dim11_rot8": lambda: _build_layout(502, D=11, rot_col=8),
    "E_f3": lambda: _build_layout(503, F=3),
    "E_f6": lambda: _build_layout(504, F=6),
    "E_nc3": lambda: _build_layout(505, classes=(3,)),
    "E_nc32": lambda: _build_layout(506, classes=(10, 10, 12)),
    "E_tail": lambda: _build_layout(507, tail_rows=100),
    "F_clean": lambda: _build_f()["clean"], "F_dirty1": lambda: _build_f()["dirty1"],
    "F_dirty2": lambda: _build_f()["dirty2"], "F_counts": lambda: _build_f()["counts"],
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The case ``name`` (one of ``NAMES``); built once per process, treat it as read-only."""
    return _BUILDERS[name]()
