"""Planted inputs for the anchor head's decode + rotated NMS (``al3d_head_decode_nms``), shared by the GPU test
(tests/test_anchorhead_fp64_gpu.py) and the CPU checks of the plants (tests/test_anchorhead_fp64_cpu.py).

A box is planted EXACTLY: it is the anchor and its ten regressions are zero, so the decode returns the anchor apart from one
``atan2f(sinf, cosf)`` round trip of the angle.  The anchor's vx carries its index and its vy its task, so a returned box
names its anchor.  Scores of a (sample, task) come from an arithmetic grid in (score_thresh + 0.05, 0.95) with spacing
>= 1e-5, handed out along an explicit or seeded rank order, logits = float32 of the float64 logit; everything else sits at
logit -8.  The anchors are shared by the samples of a call; the scores of a sample decide which planted boxes are awake in it.

Families (``FAMILIES``), each at the placements ``origin`` and ``range`` (clusters translated to (+-48, +-48) m, the sign
pair cycling over the tasks): tight_bounds, degenerate, chains, cuts_1000_83 / cuts_1024_128 and random_at_range (``range``
only).  See the builders.

THE THRESHOLD BAND.  A float32 decision may differ from the float64 one only where a float32 quantity sits on a threshold.
Its half-width for the IoU is measured, not assumed: ``measure_band`` takes every pair the yardstick evaluates in every
family and forms max |IoU_float32 - IoU_float64| with the float32 CPU oracle (``oracle.rbox_pair`` on ``oracle.box_decode``'s
boxes; never the kernel).  ``python tests/anchorhead_cases.py`` reprints the figures below; tests/test_anchorhead_fp64_cpu.py
fails when a recomputed maximum exceeds its recorded one or falls below 0.8 of it.  HOW TO RE-RECORD: whenever a plant moves
(or the oracle's arithmetic changes, for the better too) run this file and copy the printed maxima, rounded up to two digits,
into BOTH recorded constants by hand: ``MEASURED`` and ``TIGHT_MAX``.  The two interlock -- the band plants sit at
2 x 4 x TIGHT_MAX and are themselves measured pairs -- so run it again after the copy and keep the larger footprint figure
if it moved (see the comment at TIGHT_MAX); then update the figures in this docstring and in DESIGN.md's pinning section.

  Measured maxima of |IoU_f32 - IoU_f64| (MEASURED), shoelace about the polygon's first vertex (csrc/al3d_rbox.h); "other"
  are the boxes of degenerate, chains (0.5 x 1.0), cuts (0.4 x 0.4) and random_at_range:
    origin:  traffic_cone 2.4e-07  pedestrian 2.2e-07  bicycle 3.7e-07  motorcycle 3.1e-07  barrier 4.8e-07  car 2.6e-07
             truck 1.5e-07  construction_vehicle 2.0e-07  bus 2.7e-07  trailer 2.0e-07  sliver 1.4e-06  other 4.1e-06
    range:   traffic_cone 4.4e-06  pedestrian 4.0e-06  bicycle 4.6e-06  motorcycle 3.1e-06  barrier 3.5e-06  car 1.2e-06
             truck 6.5e-07  construction_vehicle 6.3e-07  bus 7.5e-07  trailer 5.0e-07  sliver 4.9e-06  other 2.5e-05
  delta = 4 x the placement's maximum (the factor covers the device's sinf / cosf differing from libm by an ulp in each
  corner):  origin 1.64e-05, range 1.0e-04.  1e-3 * thr = 2e-4: at range delta is half the kernel's 0.1 % prefilter margin,
  the measured error itself an eighth of it.  The margin holds, with that headroom.

  BEFORE the shoelace was made vertex-relative (products of absolute coordinates, ~2900 m^2 at range with an ulp of 2.4e-4)
  the same measurement gave, at range: traffic_cone 3.1e-03, pedestrian 1.6e-03, sliver 2.6e-04, car 5.9e-05, bus 1.7e-05 --
  delta = 1.2e-2 = 62 x (1e-3 * thr): the 0.1 % margin was not "for rounding" there, and a cone pair anywhere within 1.5 % of
  the threshold could be decided either way.  That is what moved csrc/al3d_rbox.h and oracle/al3d_oracle_detector.c.

  Pairs whose float64 IoU is within delta of thr are off-limits, except tight_bounds' deliberate plants at thr +- 2 delta.
  tight_bounds holds the eleven footprints only, so its band is DELTA_TIGHT = 4 x TIGHT_MAX, the largest FOOTPRINT maximum of the
  placement (origin 1.4e-6 -> 5.6e-6, range 6.5e-6 -> 2.6e-5; see TIGHT_MAX for why it is recorded apart).  It plants eps in +-{2 delta_tight / thr, 3e-4, 7e-4, 1.5e-3, 1e-2}; an eps with
  |eps| * thr < 2.5 delta_tight could not be told from the band plant and is left out: at range that is +-3e-4 alone (6e-5 absolute against
  2 delta_tight = 5.2e-5: the band plant at +-2.6e-4 stands in its place), so +-7e-4 and +-2.6e-4 probe the inside of the
  0.1 % margin there; at the origin all are planted.
  The score "an ulp below" score_thresh in cuts is 4 ulps below (logit -2^-21): float32 1 / (1 + expf(-x)) cannot give
  0.5 - 1 ulp, a logit of -2^-23 rounds back to 0.5; -2^-21 is the nearest that every faithful float32 sigmoid must drop.
  Redrawn shares (random_at_range, asserted < 1 %): see ``python tests/anchorhead_cases.py``; recorded: 0.00056.
"""
import ctypes

import numpy as np

import head_fp64 as H

F32 = lambda v: float(np.float32(v))      # noqa: E731  constants as the kernel holds them
THR = F32(0.2)
SCORE_THR = F32(0.1)
WIDE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]                       # post_center_limit_range of the CBGS configs
PLACEMENTS = {"origin": 0.0, "range": 48.0}
SIGNS = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
# BEV footprints (w, l) of the ten CBGS classes (nuScenes mean sizes) and a 20 : 1 sliver
FOOTPRINTS = {"traffic_cone": (0.41, 0.41), "pedestrian": (0.67, 0.73), "bicycle": (0.60, 1.70), "motorcycle": (0.77, 2.11),
              "barrier": (2.53, 0.50), "car": (1.97, 4.63), "truck": (2.51, 6.93), "construction_vehicle": (2.85, 6.37),
              "bus": (2.94, 10.5), "trailer": (2.90, 12.29), "sliver": (0.30, 6.0)}
# measured maxima of |IoU_f32 - IoU_f64| per placement and footprint, rounded up to two digits (module docstring)
MEASURED = {
    "origin": {"traffic_cone": 2.4e-07, "pedestrian": 2.2e-07, "bicycle": 3.7e-07, "motorcycle": 3.1e-07, "barrier": 4.8e-07, "car": 2.6e-07, "truck": 1.5e-07, "construction_vehicle": 2.0e-07, "bus": 2.7e-07, "trailer": 2.0e-07, "sliver": 1.4e-06, "other": 4.1e-06},
    "range": {"traffic_cone": 4.4e-06, "pedestrian": 4.0e-06, "bicycle": 4.6e-06, "motorcycle": 3.1e-06, "barrier": 3.5e-06, "car": 1.2e-06, "truck": 6.5e-07, "construction_vehicle": 6.3e-07, "bus": 7.5e-07, "trailer": 5.0e-07, "sliver": 4.9e-06, "other": 2.5e-05},
}
DELTA = {p: 4.0 * max(m.values()) for p, m in MEASURED.items()}
# tight_bounds holds only the eleven footprints: its band comes from their own maxima, not from the 'other' boxes of the rest
# TIGHT_MAX bounds the footprint maxima above.  It is recorded on its own because the band plants sit at 2 x 4 x TIGHT_MAX and
# so feed back into the measurement: at range the footprints measure 4.9e-6 with the plants where 6.5e-6 puts them and 6.5e-6
# where 4.9e-6 puts them; the larger is kept.
TIGHT_MAX = {"origin": 1.4e-06, "range": 6.5e-06}
DELTA_TIGHT = {p: 4.0 * v for p, v in TIGHT_MAX.items()}
EPS = [3e-4, 7e-4, 1.5e-3, 1e-2]


def eps_list(placement):
    """Relative offsets of the tight_bounds plants: +-2 delta (absolute) and every listed eps outside 2 delta."""
    d2 = 2.0 * DELTA_TIGHT[placement] / THR
    e = [d2] + [v for v in EPS if v * THR >= 2.0 * DELTA_TIGHT[placement] * 1.25]
    return [s * v for v in e for s in (1.0, -1.0)]


class Scene:
    """Anchors per task and, per (sample, task), the awake anchors in rank order."""

    def __init__(self, B, na, nc, gap=0, **params):
        self.B, self.na, self.nc, self.gap = B, list(na), list(nc), gap
        self.boxes = [[] for _ in na]                    # per task: (x, y, w, l, r, class)
        self.foot = [[] for _ in na]
        self.rank = {}                                   # (b, t) -> (anchor indices best first, scores or None)
        self.params = dict(score_thresh=SCORE_THR, iou_thresh=THR, pre_max=1000, post_max=83, rng=WIDE)
        self.params.update(params)

    def add(self, t, x, y, w, l, r, cls=None, foot="other"):
        self.boxes[t].append((x, y, w, l, r, len(self.boxes[t]) % self.nc[t] if cls is None else cls))
        self.foot[t].append(foot)
        return len(self.boxes[t]) - 1

    def wake(self, b, t, idx, scores=None):
        assert (b, t) not in self.rank
        self.rank[(b, t)] = (np.asarray(idx, np.int64), None if scores is None else np.asarray(scores, np.float64))

    def finish(self):
        """-> dict(hout [B,HW,CH] f32, anchors [A_t,9] f32 per task, na, nc, box_off, cls_off, label_off, params, foot)."""
        nt = len(self.na)
        HW = max(1, max(-(-len(bx) // na) for bx, na in zip(self.boxes, self.na)))
        box_off, cls_off, off = [], [], 0
        for t in range(nt):                              # [all box regressions | all class logits], as the fused head
            box_off.append(off)
            off += self.na[t] * 10
        for t in range(nt):
            off += self.gap if t == nt - 1 else 0        # a gap widens the class window past the staged pre-pass' limit
            cls_off.append(off)
            off += self.na[t] * self.nc[t]
        CH = off
        hout = np.zeros((self.B, HW, CH), np.float32)
        anchors = []
        thr = self.params["score_thresh"]
        for t in range(nt):
            A = HW * self.na[t]
            a = np.zeros((A, 9), np.float32)
            a[:, 2], a[:, 3], a[:, 4], a[:, 5] = -1.0, 1.0, 1.0, 1.5
            a[:, 6], a[:, 7] = np.arange(A), t
            bx = np.asarray(self.boxes[t], np.float64).reshape(-1, 6)
            n = len(bx)
            a[:n, 0], a[:n, 1], a[:n, 3], a[:n, 4], a[:n, 8] = bx[:, 0], bx[:, 1], bx[:, 2], bx[:, 3], bx[:, 4]
            anchors.append(a)
            cls = np.full((self.B, A, self.nc[t]), -8.0, np.float32)
            for b in range(self.B):
                idx, sc = self.rank.get((b, t), (np.zeros(0, np.int64), None))
                if sc is None:
                    sc = np.linspace(0.95, thr + 0.05, len(idx)) if len(idx) > 1 else np.full(len(idx), 0.9)
                    assert len(idx) < 2 or sc[0] - sc[1] >= 1e-5
                assert len(idx) == len(sc) and len(set(idx.tolist())) == len(idx) and (len(idx) == 0 or idx.max() < n)
                lg = np.log(sc / (1.0 - sc)).astype(np.float32)
                for i, v in zip(idx, lg):
                    cls[b, i, :] = v - 3.0 - np.arange(self.nc[t])
                    cls[b, i, int(bx[i, 5])] = v
            hout[:, :, cls_off[t]:cls_off[t] + self.na[t] * self.nc[t]] = cls.reshape(self.B, HW, -1)
        label_off = np.concatenate([[0], np.cumsum(self.nc)])[:-1].tolist()
        return dict(hout=hout, anchors=anchors, na=self.na, nc=self.nc, box_off=box_off, cls_off=cls_off, label_off=label_off,
                    params=dict(self.params), foot=self.foot)


def _centre(placement, t):
    sx, sy = SIGNS[t % 4]
    return sx * PLACEMENTS[placement], sy * PLACEMENTS[placement]


def _pack(radii, width=16.0):
    """Shelf-pack circles, largest first, rows at most ``width`` wide -> centres [n,2] about the packing's middle."""
    order = np.argsort(-np.asarray(radii), kind="stable")
    pos = np.zeros((len(radii), 2))
    x = y = rowh = 0.0
    for i in order:
        d = 2.0 * radii[i]
        if x > 0 and x + d > width:
            x, y, rowh = 0.0, y + rowh, 0.0
        pos[i] = (x + radii[i], y + radii[i])
        x, rowh = x + d, max(rowh, d)
    return pos - 0.5 * (pos.min(0) + pos.max(0))


# ------------------------------------------------------------------------------------------------ tight_bounds
# task = one kind of pair whose IoU EQUALS one of the kernel's upper bounds:
#   nested   concentric, same angle, inner = outer scaled by sqrt(IoU)            IoU = area ratio
#   axis     equal boxes at r in {0, pi/2, -pi/2, pi} shifted along their width   IoU = stand-up bound
#   par      equal boxes at an arbitrary r shifted along width (u) or length (v)  IoU = own-frame bound
TIGHT_KINDS = [("nested", 0.3, "u"), ("axis", 0.0, "u"), ("axis", F32(np.pi / 2), "u"), ("axis", F32(-np.pi / 2), "u"),
               ("axis", F32(np.pi), "u"), ("par", 0.7, "u"), ("par", -2.1, "v"), ("par", 1.3, "u")]
TIGHT_GROUPS = [["trailer", "traffic_cone", "pedestrian", "bicycle"], ["bus", "motorcycle", "barrier", "sliver"],
                ["truck", "construction_vehicle", "car"]]


def tight_bounds(placement):
    """Sample = (eps, footprint group, roles): sample b wakes, in every task, the pairs of group ``b % 3`` planted at
    ``eps_list[(b // 3) % ne]``; in the second half of the samples the two boxes of each pair swap ranks."""
    eps = eps_list(placement)
    ne, ng = len(eps), len(TIGHT_GROUPS)
    sc = Scene(2 * ne * ng, na=[1, 2, 1, 3, 1, 2, 1, 1], nc=[1, 2, 3, 1, 2, 1, 4, 2],
               rng=[-75.0, -75.0, -10.0, 75.0, 75.0, 10.0])      # the bus and trailer pairs reach past 61.2 m at range
    rng = np.random.default_rng(5)
    plants = {}                                          # (b, t) -> [(first anchor, second anchor, eps, kind, footprint)]
    for t, (kind, r, axis) in enumerate(TIGHT_KINDS):
        ox, oy = _centre(placement, t)
        for g, group in enumerate(TIGHT_GROUPS):
            radii = [0.5 * np.hypot(FOOTPRINTS[f][0] * (1.68 if axis == "u" else 1.0), FOOTPRINTS[f][1] * (1.68 if axis == "v" else 1.0))
                     + 0.3 for f in group]                   # a pair reaches 1.67 x its box along the shift
            pos = _pack(radii)
            for e, ep in enumerate(eps):
                iou = THR * (1.0 + ep)
                pair = []
                for f, (px, py) in zip(group, pos):
                    w, l = FOOTPRINTS[f]
                    x, y = ox + px, oy + py
                    i = sc.add(t, x, y, w, l, r, foot=f)
                    if kind == "nested":
                        j = sc.add(t, x, y, w * np.sqrt(iou), l * np.sqrt(iou), r, foot=f)
                    else:
                        d = (w if axis == "u" else l) * (1.0 - iou) / (1.0 + iou)
                        ux, uy = (np.cos(r), -np.sin(r)) if axis == "u" else (np.sin(r), np.cos(r))
                        j = sc.add(t, x + d * ux, y + d * uy, w, l, r, foot=f)
                    pair.append((i, j, ep, kind, f))
                for swap in (0, 1):
                    b = (swap * ne + e) * ng + g
                    order = rng.permutation(len(pair))
                    sc.wake(b, t, [k for q in order for k in (pair[q][:2][::-1] if swap else pair[q][:2])])
                    plants[(b, t)] = pair
    case = sc.finish()
    case["plants"] = plants
    return case


# ------------------------------------------------------------------------------------------------ degenerate
def degenerate(placement):
    sc = Scene(2, na=[1, 2, 1], nc=[2, 1, 3])
    expect = {}                                          # t -> {"suppressed": [...], "kept": [...]} by anchor index
    pi32 = F32(np.pi)
    for t in range(3):
        ox, oy = _centre(placement, t)
        spot = iter([(ox + 6.0 * (k % 5 - 2), oy + 6.0 * (k // 5 - 1.5)) for k in range(20)])
        kept, gone, first = [], [], []

        def pair(a, b, suppress):
            i, j = sc.add(t, *a), sc.add(t, *b)
            first.append((i, j))
            kept.append(i)
            (gone if suppress else kept).append(j)
        x, y = next(spot); pair((x, y, 1.9, 4.5, 0.4), (x, y, 1.9, 4.5, 0.4), True)                # the same box twice
        x, y = next(spot); pair((x, y, 2.0, 1.0, 0.0), (x + 2.0, y, 2.0, 1.0, 0.0), False)         # share an edge, exactly
        x, y = next(spot); pair((x, y, 2.0, 1.0, 0.0), (x + 2.0, y + 1.0, 2.0, 1.0, 0.0), False)   # share a corner only
        x, y = next(spot); pair((x, y, 2.0, 4.0, 0.9), (x + 2.0 * np.cos(0.9), y - 2.0 * np.sin(0.9), 2.0, 4.0, 0.9), False)
        x, y = next(spot); pair((x, y, 2.0, 4.0, -1.1), (x + 0.1, y - 0.2, 1.0, 4.0, -1.1), True)  # inside, ratio 0.5
        x, y = next(spot); pair((x, y, 2.0, 4.0, -1.1), (x + 0.1, y - 0.2, 0.4, 2.0, -1.1), False)  # inside, ratio 0.1
        x, y = next(spot); pair((x, y, 0.8, 2.1, 0.6), (x, y, 0.8, 2.1, F32(0.6) + np.pi), True)   # r and r + pi
        x, y = next(spot); pair((x, y, 0.8, 2.1, pi32), (x, y, 0.8, 2.1, -pi32), True)             # r = +-pi exactly
        x, y = next(spot); pair((x, y, 0.6, 1.7, 40.0), (x, y, 0.6, 1.7, 40.0 - 12 * np.pi), True)  # |r| = 40
        x, y = next(spot); pair((x, y, 0.6, 1.7, -40.0), (x, y, 0.5, 0.5, -40.0), True)            # ... nested, ratio 0.245
        x, y = next(spot); pair((x, y, 2.0, 4.0, 0.0), (x + 0.3, y, 0.0, 3.0, 0.0), False)         # zero width inside a box
        x, y = next(spot); pair((x, y, 2.0, 4.0, 0.5), (x, y + 0.2, 0.0, 3.0, -0.7), False)        # ... rotated
        x, y = next(spot); pair((x, y, np.nan, 4.0, 0.2), (x + 0.2, y, 2.0, 4.0, 0.2), False)      # NaN width on top of a box
        x, y = next(spot); pair((np.nan, y, 2.0, 4.0, 0.2), (x, y, 2.0, 4.0, 0.2), False)          # NaN x; y overlaps
        x, y = next(spot); pair((x, y, 2.0, 4.0, np.nan), (x + 0.2, y, 2.0, 4.0, 0.2), False)      # NaN angle: centre stays
        if placement == "origin":
            # IoU == thr in float64 AND in float32: a 1 x 1 box at (0, 0) and a thr x 1 box inside it.  The corners (+-0.5,
            # +-thr / 2) are exact; the clip keeps the inner box's four vertices as they are (its edge tests, e.g. 0.5 - thr / 2,
            # ARE rounded, but only their signs are used and no crossing point is formed); the shoelace about the first vertex
            # multiplies thr by 1; (1 + thr) - thr rounds to 1 in both formats.  So inter / union = thr wherever the arithmetic
            # is IEEE: separate multiply and add (no contraction into FMA) and a correctly rounded division.  If this plant
            # flips, look for -ffast-math, a dropped -ffp-contract=off or an approximate division first.  ``>=`` suppresses
            # where ``>`` would not.  The one plant ON the threshold; off the origin the corners would not be exact.
            pair((0.0, 0.0, 1.0, 1.0, 0.0), (0.0, 0.0, THR, 1.0, 0.0), True)
        expect[t] = dict(kept=kept, suppressed=gone, nan_centre=[first[12][0], first[13][0]],   # NaN w -> NaN diagonal -> NaN centre
                         nan_angle=first[14][0], on_threshold=first[-1] if placement == "origin" else None)
        rng = np.random.default_rng(3 + t)
        order = rng.permutation(len(first))
        sc.wake(0, t, [k for q in order for k in first[q]])                    # the first of each pair outranks the second
        sc.wake(1, t, [p[0] for p in first] + [first[q][1] for q in order])    # all firsts (NaN ones too) ahead of all seconds
    case = sc.finish()
    case["expect"] = expect
    return case


# ------------------------------------------------------------------------------------------------ chains
CHAIN_LENGTHS = [2, 3, 8, 9, 17, 40]


def chains(placement):
    """Rows of 0.5 x 1.0 boxes at r = 0.3, neighbours shifted along the width so that IoU(k, k+1) = 0.4 and
    IoU(k, k+2) = 0.077; a clique of 30 nearly coincident boxes.  Rank orders: along the rows; round-robin over the rows;
    seeded; each row backwards."""
    sc = Scene(2, na=[1, 3, 2, 1], nc=[1, 2, 1, 3], gap=160)
    r, w, l = 0.3, 0.5, 1.0
    d = w * (1.0 - 0.4) / (1.0 + 0.4)
    rows_of = {}
    for t in range(4):
        ox, oy = _centre(placement, t)
        rows = []
        for q, n in enumerate(CHAIN_LENGTHS):
            x0, y0 = ox - 4.5 + 1.6 * q * np.sin(r), oy + 1.6 * (q - 2.5) * np.cos(r)
            rows.append([sc.add(t, x0 + k * d * np.cos(r), y0 - k * d * np.sin(r), w, l, r) for k in range(n)])
        rng = np.random.default_rng(11 + t)
        clique = [sc.add(t, ox + 6.0 + rng.uniform(-0.02, 0.02), oy + 6.0 + rng.uniform(-0.02, 0.02), 0.8, 0.8,
                         0.1 + rng.uniform(-0.02, 0.02)) for _ in range(30)]
        rows_of[t] = (rows, clique)
        flat = [k for row in rows for k in row]
        robin = [row[k] for k in range(max(CHAIN_LENGTHS)) for row in rows if k < len(row)]
        orders = [flat + clique, robin + clique, list(rng.permutation(flat + clique)), [k for row in rows for k in row[::-1]] + clique]
        sc.wake(0, t, orders[t])
        sc.wake(1, t, orders[(t + 1) % 4])
    case = sc.finish()
    case["rows"] = rows_of
    return case


# ------------------------------------------------------------------------------------------------ cuts
def cuts(placement, pre_max, post_max):
    """score_thresh = 0.5 (float32 sigmoid(0) is 0.5 exactly).
    task 0: 1100 separate boxes, a run of 50 equal scores at ranks 990..1039; the post_max cut falls inside a super-round.
    task 1: ranks 1..989 are 30 cliques, the rest are separate boxes with the same run of equal scores: the survivors after the
            cliques' 30 are exactly the separate boxes that pre_max let in -- the run's lowest anchor indices.
    task 2: a score equal to the threshold (kept), one just below (logit -2^-21, float64 score 0.5 - 1.2e-7: dropped by every
            faithful float32 sigmoid), and pairs whose better box lies outside the limit range and still suppresses.
    task 3: nothing awake.  task 4: one box."""
    ox, oy = PLACEMENTS[placement], -PLACEMENTS[placement]
    limit = [ox - 8.0, oy - 8.0, -10.0, ox + 2.05, oy + 8.0, 10.0]
    sc = Scene(1, na=[2, 1, 1, 1, 2], nc=[1, 2, 3, 1, 2], score_thresh=F32(0.5), pre_max=pre_max, post_max=post_max, rng=limit)
    rng = np.random.default_rng(pre_max)
    n = 1100
    scores = np.linspace(0.95, 0.56, n)
    scores[989:1039] = scores[989]
    cells = rng.permutation(34 * 34)[:n]                 # anchor index <-> position and <-> rank: both shuffled
    idx0 = [sc.add(0, ox + 0.6 * (c % 34 - 16.5), oy + 0.6 * (c // 34 - 16.5), 0.4, 0.4, rng.uniform(-3, 3)) for c in cells]
    order0 = rng.permutation(idx0)
    sc.wake(0, 0, order0, scores)
    where = rng.permutation(n)                           # anchor slot of the k-th planted box
    geo = [None] * n
    for k in range(989):
        q = k % 30
        geo[where[k]] = (ox + 1.5 * (q % 6 - 2.5) + rng.uniform(-0.01, 0.01), oy + 6.0 + 1.5 * (q // 6) + rng.uniform(-0.01, 0.01),
                         0.4, 0.4, 0.5 + rng.uniform(-0.01, 0.01))
    for k in range(989, n):
        q = k - 989
        geo[where[k]] = (ox + 0.6 * (q % 20 - 9.5), oy - 6.0 + 0.6 * (q // 20), 0.4, 0.4, rng.uniform(-3, 3))
    for g in geo:
        sc.add(1, *g)
    sc.wake(0, 1, where, scores)
    s2, i2 = [], []
    for k in range(6):                                   # the better box is outside the limit range (x or y), its partner inside
        inside = (ox + 1.9 - 0.3 * (k % 2), oy + 2.0 * (k - 2.5))
        out = (inside[0] + 0.3, inside[1]) if k % 2 == 0 else (ox + 3.0 + k, oy)
        a = sc.add(2, out[0], out[1], 1.0, 2.0, 0.0)
        b = sc.add(2, (out[0] if k % 2 == 0 else inside[0]) - (0.2 if k % 2 == 0 else 0.0), inside[1], 1.0, 2.0, 0.0)
        i2 += [a, b]
        s2 += [0.9 - 0.01 * k, 0.7 - 0.01 * k]
    at, below = sc.add(2, ox - 5.0, oy - 5.0, 1.0, 1.0, 0.3), sc.add(2, ox - 5.0, oy + 5.0, 1.0, 1.0, 0.3)
    sc.wake(0, 2, i2 + [at, below], s2 + [0.5, 0.5])
    sc.add(3, ox, oy, 1.0, 1.0, 0.0)
    sc.wake(0, 4, [sc.add(4, ox - 1.0, oy + 1.0, 2.0, 4.0, 0.3)])
    case = sc.finish()
    c2 = case["hout"][0, :, case["cls_off"][2]:case["cls_off"][2] + 3]
    c2[below] = np.float32(-2.0 ** -21) - 3.0 - np.arange(3)
    c2[below, below % 3] = np.float32(-2.0 ** -21)
    assert c2[at].max() == 0.0
    case["marks"] = dict(at=at, below=below, tie_run={0: order0[989:1039], 1: where[989:1039]})
    return case


# ------------------------------------------------------------------------------------------------ random_at_range
def random_at_range(placement="range", seed=0):
    """600 boxes per task, drawn like centerhead_cases._draw_geometry (w 1.5..5, l 0.6..2.2, any angle) in 100 clusters of 6
    with centres uniform over +-50 m; the later box of a pair within delta of the threshold is redrawn."""
    assert placement == "range"
    rng = np.random.default_rng(seed)
    na, nc, n = [1, 2, 3], [2, 1, 4], 600
    delta = DELTA["range"]

    def draw(c):
        return (c[0] + rng.normal(0, 0.8), c[1] + rng.normal(0, 0.8), rng.uniform(1.5, 5.0), rng.uniform(0.6, 2.2), rng.uniform(-np.pi, np.pi))
    centres = [rng.uniform(-50, 50, (100, 2)) for _ in na]
    geo = [[draw(centres[t][k // 6]) for k in range(n)] for t in range(len(na))]
    orders = {(b, t): rng.permutation(n) for b in range(2) for t in range(len(na))}
    redrawn = set()
    for _ in range(20):
        sc = Scene(2, na=na, nc=nc)
        for t in range(len(na)):
            for g in geo[t]:
                sc.add(t, *g)
        for (b, t), o in orders.items():
            sc.wake(b, t, o)
        case = sc.finish()
        ref, pairs = expected(case, want_pairs=True)
        bad = {(t, int(ref[b][t]["cand"][j])) for (b, t), pl in pairs.items() for i, j, q in pl if abs(q["iou"] - THR) < delta}
        if not bad:
            break
        for t, k in bad:
            geo[t][k] = draw(centres[t][k // 6])
            redrawn.add((t, k))
    else:
        raise AssertionError("the geometry repair did not converge")
    case["redrawn_share"] = len(redrawn) / (n * len(na))
    case["overlapping_pairs"] = {k: sum(1 for _, _, q in pl if q["iou"] > 0) for k, pl in pairs.items()}
    case["ref"], case["pairs"] = ref, pairs
    return case


FAMILIES = {"tight_bounds": tight_bounds, "degenerate": degenerate, "chains": chains,
            "cuts_1000_83": lambda p: cuts(p, 1000, 83), "cuts_1024_128": lambda p: cuts(p, 1024, 128),
            "random_at_range": random_at_range}
CASES = [(f, p) for f in FAMILIES for p in PLACEMENTS if not (f == "random_at_range" and p == "origin")]
_cache = {}


def make(family, placement):
    """-> (case, yardstick result [b][t], pairs {(b, t): [(i, j, quantities)]}); built once per process, never changed."""
    key = (family, placement)
    if key not in _cache:
        case = FAMILIES[family](placement)
        ref, pairs = (case["ref"], case["pairs"]) if "ref" in case else expected(case, want_pairs=True)
        _cache[key] = (case, ref, pairs)
    return _cache[key]


def expected(case, want_pairs=False, strict=False):
    """The float64 yardstick on a case -> [[task_predict dict per task] per sample] (, pairs)."""
    p, pairs, out = case["params"], {}, []
    for b in range(case["hout"].shape[0]):
        row = []
        for t in range(len(case["na"])):
            row.append(H.task_predict(case["hout"][b], case["anchors"][t], case["na"][t], case["nc"][t], case["box_off"][t],
                                      case["cls_off"][t], p["score_thresh"], p["iou_thresh"], p["pre_max"], p["post_max"],
                                      p["rng"], pairs.setdefault((b, t), []) if want_pairs else None, strict))
        out.append(row)
    return (out, pairs) if want_pairs else out


def run_library(case, sentinel=-7777.0):
    """``al3d_head_decode_nms`` on the case the way models/bbox_heads.py calls it -> (boxes [B,nt,post,9], scores, labels, counts)
    as numpy arrays; the outputs are pre-filled with ``sentinel``."""
    import torch
    from al3d import lib
    dev = torch.device("cuda:0")
    p = case["params"]
    hout = torch.from_numpy(case["hout"]).to(dev).contiguous()
    B, HW, CH = hout.shape
    nt, post = len(case["na"]), p["post_max"]
    a_dev = [torch.from_numpy(a).to(dev).contiguous() for a in case["anchors"]]
    boxes = torch.full((B, nt, post, 9), sentinel, dtype=torch.float32, device=dev)
    scores = torch.full((B, nt, post), sentinel, dtype=torch.float32, device=dev)
    labels = torch.full((B, nt, post), int(sentinel), dtype=torch.int32, device=dev)
    counts = torch.full((B, nt), int(sentinel), dtype=torch.int32, device=dev)
    IntA = ctypes.c_int * nt
    task_a = IntA(*[a.shape[0] for a in a_dev])
    ws = torch.empty(lib.load().al3d_head_decode_nms_workspace_bytes(B, nt, task_a), dtype=torch.uint8, device=dev)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
    lib.call("al3d_head_decode_nms", vp(hout), B, HW, CH, nt, (ctypes.c_void_p * nt)(*[a.data_ptr() for a in a_dev]), task_a,
             IntA(*case["na"]), IntA(*case["nc"]), IntA(*case["box_off"]), IntA(*case["cls_off"]), IntA(*case["label_off"]),
             float(p["score_thresh"]), float(p["iou_thresh"]), int(p["pre_max"]), post,
             (ctypes.c_float * 6)(*[float(v) for v in p["rng"]]), vp(boxes), vp(scores), vp(labels), vp(counts), vp(ws),
             torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy()


def compare(case, ref, got, sentinel=-7777.0):
    """Assert the library's output equals the yardstick's: kept anchors and their order exactly, labels with label_off, scores
    to 2e-7, boxes to 1e-6 relative, the angle to 2e-6 modulo 2 pi, counts, and untouched rows past counts."""
    boxes, scores, labels, counts = got
    for b, row in enumerate(ref):
        for t, r in enumerate(row):
            k = len(r["anchors"])
            where = f"sample {b} task {t}"
            assert counts[b, t] == k, (where, int(counts[b, t]), k)
            assert np.all(boxes[b, t, k:] == sentinel) and np.all(scores[b, t, k:] == sentinel) and \
                np.all(labels[b, t, k:] == int(sentinel)), where + ": rows past counts were written"
            gb = boxes[b, t, :k].astype(np.float64)
            assert gb[:, 6].astype(np.int64).tolist() == r["anchors"].tolist(), (where, gb[:, 6].tolist(), r["anchors"].tolist())
            assert np.all(gb[:, 7] == t), where
            assert labels[b, t, :k].tolist() == (r["labels"] + case["label_off"][t]).tolist(), where
            assert np.all(np.abs(scores[b, t, :k] - r["scores"]) <= 2e-7), (where, np.abs(scores[b, t, :k] - r["scores"]).max())
            rb = r["boxes"]
            same_nan = np.isnan(gb[:, :8]) == np.isnan(rb[:, :8])
            close = np.abs(gb[:, :8] - rb[:, :8]) <= 1e-6 * np.abs(rb[:, :8])
            assert np.all(same_nan & (close | np.isnan(rb[:, :8]))), where + ": boxes differ"
            assert np.array_equal(np.isnan(gb[:, 8]), np.isnan(rb[:, 8])), where
            d = (np.abs(gb[:, 8] - rb[:, 8]) % (2 * np.pi))[~np.isnan(rb[:, 8])]
            assert np.all(np.minimum(d, 2 * np.pi - d) <= 2e-6), (where, "angle", d.max() if len(d) else 0)


def measure_band(oracle, cases=None):
    """-> {placement: {footprint: max |IoU_f32 - IoU_f64|}} over every pair the yardstick evaluates (float32 = the CPU oracle's
    decode + pair geometry)."""
    out = {p: {} for p in PLACEMENTS}
    for family, placement in (cases or CASES):
        case, ref, pairs = make(family, placement)
        for (b, t), pl in pairs.items():
            if not pl:
                continue
            cand = ref[b][t]["cand"]
            a = case["anchors"][t][cand]
            hw = case["hout"].shape[1]
            enc = case["hout"][b][:, case["box_off"][t]:case["box_off"][t] + case["na"][t] * 10].reshape(hw * case["na"][t], 10)[cand]
            b32 = oracle.box_decode(enc, a)[:, [0, 1, 3, 4, 8]]
            for i, j, q in pl:
                err = abs(oracle.rbox_pair(b32[i], b32[j])[3] - q["iou"])
                f = case["foot"][t][cand[i]]
                out[placement][f] = max(out[placement].get(f, 0.0), err)
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import oracle
    oracle.build()
    for placement, m in measure_band(oracle).items():
        print(placement, " ".join(f"{f} {m.get(f, 0.0):.1e}" for f in MEASURED[placement]))
        print(f"  delta recorded {DELTA[placement]:.2e}, 4 x measured maximum {4 * max(m.values()):.2e}, 1e-3 * thr {1e-3 * THR:.1e};"
              f" tight_bounds: delta recorded {DELTA_TIGHT[placement]:.2e}, eps planted {sorted(set(abs(e) for e in eps_list(placement)))}")
    case = make("random_at_range", "range")[0]
    print("random_at_range: redrawn share", f"{case['redrawn_share']:.5f}", "pairs with IoU > 0:", case["overlapping_pairs"])
