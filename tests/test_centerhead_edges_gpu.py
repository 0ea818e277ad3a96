"""GPU suite for the decisions of the CenterHead post-processing kernel (csrc/center_head.hip: ``center_score_kernel``,
``center_nms_kernel``) that tests/test_centerhead_gpu.py stays off by construction.  ``detector_ops.center_decode_nms``
runs the hand-built cases of tests/centerhead_edge_cases.py; counts, labels, order, scores and boxes are compared with
BOTH the hand-written expectation and the float64 yardstick tests/center_fp64.py (that the two agree exactly is
tests/test_centerhead_edge_cases_cpu.py).  Rows at or behind ``counts[b, t]`` are never looked at.

Cases:
  ties        every cell of a 5 x 7 map equal (35 cells < 1024 threads), as handed and transposed with ``swapped=False``;
              100 equal scores across the K = 64 cut of a 40 x 53 map (chunk 3, idle threads), neighbours 2^-14 apart;
              equal scores in classes 2 and 0 of a 3-class task (24 candidates padded to 32) and of a 4-class task (32)
  thresholds  score == coder threshold dropped, one ulp below kept; score == test threshold kept on the rotate path, one
              ulp above dropped, not applied on the circle path; ``None`` / ``0`` filter nothing (score-0 background comes out)
  ranges      a centre on each of the six bounds of ``post_center_range`` kept; one ulp and one exact step outside dropped;
              the same for ``post_center_limit_range`` on the rotate path; ignored on the circle path; ``None`` and ``[]``;
              a box outside the limit range suppresses its neighbour before it is dropped
  NMS         circle: d2 == radius suppresses (3-4-5, radius 25), one ulp below keeps; rotate: IoU == nms_thr keeps,
              one ulp below suppresses; identical boxes; zero-area boxes (the max(union, 1e-8) path); a per-class
              ``nms_scale``; a chain A > B > C on both paths
  cuts        ``pre_max_size`` below the survivors, before the NMS, rotate only; ``post_max_size`` reached with live
              candidates behind it, 1, and 512 of 600
  sizes       max_num 1024 x 2 classes on 32 x 32 (CT_MAXK, CT_MAXCAND, max_num == cells); 512 x 4 classes (CT_MAXCLS);
              max_num 1; 8 tasks x 2 samples with two tasks that keep nothing; one task; B = 0; every refusal
  non-finite  NaN heat logits give the bits of the same map with -inf (the kernel's NaN -> 0 key rule; the reference's
              torch.topk would rank NaN first: this pins the device rule, not the reference's); +inf scores exactly 1 and
              comes first; a NaN centre or height is dropped by the closed range and disturbs nothing else
  every case runs twice: identical bits within the counts.

Exact comparisons, and why.  One cell is 1 m (out_size_factor 8 x voxel 0.125), pc_range is integral, ``reg`` offsets
are binary fractions, ``norm_bbox=False`` leaves integral dimensions, ``rot = (0, 1)`` gives atan2f = 0, height and
velocity are copied, the merged z subtracts half an integer: every box value is a small dyadic rational that float32
holds, so boxes and labels are asserted bit for bit.  Scores of logits 0, -inf and +inf are exactly 0.5, 0 and 1 and
asserted bit for bit; the other scores go through expf and keep ``_compare``'s bound of tests/test_centerhead_gpu.py,
4u, against scores at least 1e-5 apart.  Thresholds are float32 values one ulp either side of an exact quantity.

``quad_intersection_area`` (csrc/al3d_rbox.h) on axis-aligned dyadic corners: EXACT, argued from the code.  At angle 0
``box_corners`` adds +-w/2, +-l/2 to the centre (cosf(0) = 1, sinf(0) = 0): dyadic corners.  An edge vector (ex, ey) has
one zero component, so the side value d = ex * (py - by) - ey * (px - bx) is one product of two short dyadic numbers:
exact.  A crossing point is p + tt * (q - p) with tt = d1 / (d1 - d2), the ratio in which the clip line divides an edge
of the subject box; it is exact when that ratio is dyadic, which holds for the 2 x 2 box inside the 4 x 2 box (eighths)
used for IoU == 0.5 in both clip orders.  The shoelace then sums products of dyadic differences: exact; the IoU is one
correctly rounded division of 4 by 8.  The issue's example, two 3 x 1 boxes overlapping by 2 x 1, has tt = 1/3 and 2/3,
which are NOT exact; the crossing still lands on the integer because 3 * fl(1/3) and 3 * fl(2/3) round to 1 and 2 in
float32 and in float64.  That is arithmetic, not structure, so the CPU test runs the routine restated operation for
operation in both types and asserts 0.5 exactly for all three pairs; the pair is kept as a third bracket.
"""
import numpy as np
import pytest
import torch

import center_fp64 as C
import centerhead_edge_cases as EC

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def launch(h, c, **over):
    from al3d import detector_ops as D
    out = D.center_decode_nms(torch.from_numpy(h).cuda(), c["task_ncls"], c["chan"], **dict(c["p"], **over))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_within_counts(a, b):
    assert np.array_equal(a[3], b[3]), "counts differ"
    n = a[3]
    for s in range(n.shape[0]):
        for t in range(n.shape[1]):
            for x, y in zip(a[:3], b[:3]):
                assert np.array_equal(bits(x[s, t, :n[s, t]]), bits(y[s, t, :n[s, t]])), (s, t)


def compare(got, rows, name, exact_scores=None):
    """``rows``: the expectation's (with ``exact``) or the yardstick's [[dict(boxes, scores, labels)]]."""
    boxes, scores, labels, counts = got
    assert counts.shape == (len(rows), len(rows[0])) and counts.dtype == np.int32
    for b, row in enumerate(rows):
        for t, r in enumerate(row):
            n = len(r["scores"])
            assert int(counts[b, t]) == n, (name, b, t, "count", int(counts[b, t]), n)
            assert np.array_equal(labels[b, t, :n], r["labels"]), (name, b, t, "labels / order")
            want = r["boxes"].astype(np.float32)
            assert np.array_equal(want.astype(np.float64), r["boxes"])
            assert np.array_equal(bits(boxes[b, t, :n]), bits(want)), (name, b, t, "boxes / order")
            err = np.abs(scores[b, t, :n].astype(np.float64) - r["scores"])
            assert np.all(err <= 4 * U), (name, b, t, "scores")
            exact = r["exact"] if "exact" in r else exact_scores[b][t]
            assert np.array_equal(bits(scores[b, t, :n][exact]), bits(r["scores"][exact].astype(np.float32))), (name, b, t, "exact scores")


@pytest.mark.parametrize("name", EC.NAMES)
def test_case_matches_expectation_and_yardstick(name):
    c = EC.case(name)
    got = launch(c["h"], c)
    want = EC.expected_rows(c)
    for b, row in enumerate(want):
        print(name, "sample", b, "expected per task", [len(r["scores"]) for r in row], "device", got[3][b].tolist())
    compare(got, want, name)
    ref = C.postprocess(c["h"], c["task_ncls"], c["chan"], **c["p"])
    compare(got, ref, name, exact_scores=[[r["exact"] for r in row] for row in want])
    same_within_counts(got, launch(c["h"], c))                      # determinism
    if c["h_nan"] is not None:                                      # NaN heat logits rank as -inf
        assert np.isnan(c["h_nan"]).sum() == 4
        nan = launch(c["h_nan"], c)
        same_within_counts(got, nan)
        same_within_counts(nan, launch(c["h_nan"], c))


def test_single_task_of_a_many_task_map():
    """One task per call: each task of the 8-task case on its own gives that task's rows (labels unmerged)."""
    c = EC.case("tasks_8_b2")
    whole = launch(c["h"], c, merge=False)
    for t in (0, 3, 5):
        one = dict(c, task_ncls=[c["task_ncls"][t]], chan=[c["chan"][t]])
        p = dict(merge=False, nms_type=c["p"]["nms_type"][t], nms_scale=[c["p"]["nms_scale"][t]], min_radius=[c["p"]["min_radius"][t]])
        got = launch(c["h"], one, **p)
        same_within_counts([a[:, t:t + 1] for a in whole], got)
        assert got[3].tolist() == [[len(c["expect"][b][t])] for b in range(2)]


def test_empty_batch_gives_empty_tensors():
    from al3d import detector_ops as D
    c = EC.case("tasks_8_b2")
    h = torch.from_numpy(c["h"][:0]).cuda()
    boxes, scores, labels, counts = D.center_decode_nms(h, c["task_ncls"], c["chan"], **c["p"])
    torch.cuda.synchronize()
    assert boxes.shape == (0, 8, 4, 9) and scores.shape == (0, 8, 4) and labels.shape == (0, 8, 4) and counts.shape == (0, 8)
    assert boxes.dtype == scores.dtype == torch.float32 and labels.dtype == counts.dtype == torch.int32


def _refusals():
    sc = EC.refusal_scene()
    CH = sc.CH
    window = [list(sc.chan[0])]
    window[0][3] = CH - 2                                           # dim needs three channels
    five, nine, three = EC.Scene(33, 32, [5]), EC.Scene(4, 4, [1] * 9), EC.Scene(33, 32, [3])
    three.plant(5, 0.0)
    return {
        "5_classes": (five, {}, None),
        "max_num_1025": (sc, dict(max_num=1025), None),
        "3_classes_x_700": (three, dict(max_num=700), None),
        "post_max_513": (sc, dict(post_max_size=513), None),
        "post_max_0": (sc, dict(post_max_size=0), None),
        "9_tasks": (nine, {}, None),
        "pre_max_0": (sc, dict(pre_max_size=0), None),
        "channel_window": (sc, {}, window),
    }


@pytest.mark.parametrize("name", ["5_classes", "max_num_1025", "3_classes_x_700", "post_max_513", "post_max_0", "9_tasks", "pre_max_0",
                                  "channel_window"])
def test_refusals_are_clean_errors(name):
    """Every limit one past its end: an ``Al3dError`` from the library's argument checks, which stand before the launch;
    the next valid call on the same map works."""
    from al3d import detector_ops as D, lib
    sc, over, chan = _refusals()[name]
    h = torch.from_numpy(sc.map()).cuda()
    with pytest.raises(lib.Al3dError, match="al3d_center_decode_nms_f32"):
        D.center_decode_nms(h, sc.task_ncls, chan or sc.chan, **sc.params(**over))
    torch.cuda.synchronize()
    if name not in ("5_classes", "9_tasks"):
        counts = D.center_decode_nms(h, sc.task_ncls, sc.chan, **sc.params())[3]
        assert counts.cpu().tolist() == [[1]]


def test_bad_nms_type_is_refused_by_the_wrapper():
    from al3d import detector_ops as D
    sc = EC.refusal_scene()
    h = torch.from_numpy(sc.map()).cuda()
    for bad in ("nms", ["rotate", "circle"], [None]):
        with pytest.raises(NotImplementedError, match="nms_type"):
            D.center_decode_nms(h, sc.task_ncls, sc.chan, **sc.params(nms_type=bad))
