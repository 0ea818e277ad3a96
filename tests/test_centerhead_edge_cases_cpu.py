"""CPU checks of the CenterHead edge cases (tests/centerhead_edge_cases.py): the float64 yardstick tests/center_fp64.py
alone reproduces every hand-written expectation EXACTLY -- kept cells, labels, order, and the boxes and scores gathered
from the inputs, bit for bit in float64 -- so the GPU test (tests/test_centerhead_edges_gpu.py) is judged by two
independent statements of the answer.  Also checked here: that the inputs are what the exactness argument needs
(every compared value a float32; distinct scores far enough apart), that the limits the cases reach are the kernel's,
and that the rotated-NMS pairs have their stated IoU exactly in float32 AND float64 arithmetic, by running
``quad_intersection_area`` of csrc/al3d_rbox.h restated operation for operation in either type.

Flipping any comparison of the yardstick (score > coder threshold, score >= test threshold, the closed ranges,
IoU > nms_thr, d2 <= radius) makes ``test_yardstick_reproduces_the_expectation`` fail."""
import os
import re

import numpy as np
import pytest

import center_fp64 as C
import centerhead_edge_cases as EC

U = 2.0 ** -24


def yardstick(c):
    return C.postprocess(c["h"], c["task_ncls"], c["chan"], **c["p"])


@pytest.mark.parametrize("name", EC.NAMES)
def test_yardstick_reproduces_the_expectation(name):
    c = EC.case(name)
    ref, want = yardstick(c), EC.expected_rows(c)
    assert len(ref) == len(want) == c["h"].shape[0]
    for b, (rrow, wrow) in enumerate(zip(ref, want)):
        assert len(rrow) == len(wrow) == len(c["task_ncls"])
        for t, (r, w) in enumerate(zip(rrow, wrow)):
            where = (name, b, t)
            assert r["cells"].tolist() == w["cells"].tolist(), where
            assert r["labels"].tolist() == w["labels"].tolist(), where
            assert np.array_equal(r["boxes"], w["boxes"]), where
            assert np.array_equal(r["scores"], w["scores"]), where
            # what the GPU test compares bit for bit is a float32 value on both sides
            assert np.array_equal(w["boxes"], w["boxes"].astype(np.float32).astype(np.float64)), where
            s = w["scores"][w["exact"]]
            assert np.array_equal(s, s.astype(np.float32).astype(np.float64)), where


@pytest.mark.parametrize("name", EC.NAMES)
def test_inputs_are_float32_exact_and_scores_are_ordered_alike(name):
    """Thresholds and geometry are float32 values as handed over; two different finite logits of one task give float64
    scores at least 1e-5 apart, 20 times the two float32 sigmoid errors (4u each) that could swap them."""
    c = EC.case(name)
    p = c["p"]
    assert c["h"].dtype == np.float32 and c["h"].flags["C_CONTIGUOUS"]
    vals = [p["nms_thr"], p["score_threshold"], p["coder_score_threshold"] or 0.0] + list(p["post_center_range"]) + \
        list(p["post_center_limit_range"] or []) + list(p["min_radius"]) + list(p["pc_range"]) + list(p["voxel_size"])
    assert all(float(np.float32(v)) == float(v) for v in vals)
    B, D0, D1, CH = c["h"].shape
    for t, ncls in enumerate(c["task_ncls"]):
        heat = c["chan"][t][0]
        for b in range(B):
            lg = np.unique(c["h"][b, :, :, heat:heat + ncls])
            lg = lg[np.isfinite(lg)]
            if len(lg) > 1:
                assert np.diff(C.sigmoid(lg)).min() >= 1e-5 > 20 * 8 * U, (name, b, t)


def test_limits_mirror_the_kernel():
    from al3d import detector_ops as D
    src = open(os.path.join(os.path.dirname(D.__file__), "csrc", "center_head.hip")).read()
    for k, v in EC.LIMITS.items():
        assert int(re.search(rf"^#define {k} (\d+)", src, re.M).group(1)) == v, k
    shape = lambda n: (EC.case(n)["h"].shape[1] * EC.case(n)["h"].shape[2], EC.case(n)["task_ncls"], EC.case(n)["p"])      # noqa: E731
    hw, ncls, p = shape("maxcand_2x1024")
    assert p["max_num"] == EC.LIMITS["CT_MAXK"] == hw and ncls[0] * p["max_num"] == EC.LIMITS["CT_MAXCAND"]
    assert p["post_max_size"] == EC.LIMITS["CT_MAXPOST"]
    hw, ncls, p = shape("k512_4_classes")
    assert ncls == [EC.LIMITS["CT_MAXCLS"]] and ncls[0] * p["max_num"] == EC.LIMITS["CT_MAXCAND"]
    assert hw % EC.LIMITS["CT_THREADS"] and hw < EC.LIMITS["CT_THREADS"]
    hw, ncls, p = shape("all_cells_tied_32x32")
    assert hw == p["max_num"] == EC.LIMITS["CT_MAXK"]
    assert len(EC.case("tasks_8_b2")["task_ncls"]) == EC.LIMITS["CT_MAXTASKS"] and EC.case("tasks_8_b2")["h"].shape[0] == 2
    hw, ncls, p = shape("ties_class_5x7_swapped")
    assert hw == 35 < EC.LIMITS["CT_THREADS"]
    hw, ncls, p = shape("ties_kcut_40x53")
    assert -(-hw // EC.LIMITS["CT_THREADS"]) == 3 and hw % 3                     # chunk 3, a ragged last owner, idle threads
    # bitonic padding: 24 -> 32 (padded), 32 (none), 2 (K = 1), 600 -> 1024, 2048 (none)
    t3 = EC.case("ties_classes_3_and_4")
    assert [n * t3["p"]["max_num"] for n in t3["task_ncls"]] == [24, 32]


def test_rotated_pairs_have_their_iou_exactly_in_both_precisions():
    for a, b, iou in EC.IOU_PAIRS:
        for dt in (np.float32, np.float64):
            got = EC.axis_iou(a, b, dt)
            assert type(got) is dt and float(got) == iou, (a, b, dt)
        # the yardstick's own clip states the same
        assert C.bev_iou(a + (0.0,), b + (0.0,)) == iou
    # one float32 ulp below the IoU is a threshold the pair exceeds in both precisions
    assert 0.5 > EC.below(0.5) == 0.5 - 2.0 ** -25
    # the off-threshold pairs of the other cases, for the record: exact intersections, a rounded quotient far from nms_thr
    for a, b, inter, union, thr in (((2.5, 4.5, 2, 2), (3.0, 4.5, 2, 2), 3, 5, 0.5), ((2.5, 4.5, 2, 2), (3.5, 4.5, 2, 2), 2, 6, 0.5),
                                    ((1.5, -2.5, 4, 4), (1.5, -1.75, 4, 4), 13, 19, 0.5), ((2.5, 2.5, 4, 4), (5.0, 2.5, 4, 4), 6, 26, 0.125)):
        for dt in (np.float32, np.float64):
            assert float(EC.axis_iou(a, b, dt)) == float(dt(inter) / dt(union))
        assert abs(inter / union - thr) > 0.05


def test_cases_reach_what_they_exist_for():
    """The properties the expectations lean on, computed from the inputs."""
    # the K cut falls inside the ties, and its neighbours share two leading key bytes: the select runs to its last passes
    c = EC.case("ties_kcut_40x53")
    heat = c["chan"][0][0]
    lg = c["h"][0, :, :, heat].ravel()
    keys = C.sigmoid(lg[np.isfinite(lg)]).astype(np.float32).view(np.uint32)
    assert (lg == 0).sum() == 100 and (lg > 0).sum() == 40 and (np.isfinite(lg) & (lg < 0)).sum() == 30
    # (0.5 is 0x3f000000 and a step of 2^-14 is bit 10: the first two passes see two bins, the third pass decides the cut)
    assert len(set(int(k) >> 16 for k in keys)) <= 2 and len(set((int(k) >> 8) & 0xFF for k in keys if k >= 0x3F000000)) >= 30
    tied = np.nonzero(lg == 0)[0]
    owners = tied // 3                                           # chunk 3: the thread that owns a cell
    assert len(set(owners // 64)) >= 8 and (np.diff(tied) == 1).any() and tied[0] == 0 and tied[-1] == 2119
    taken = [cell for cell, _ in c["expect"][0][0][40:]]
    assert taken == tied[:24].tolist() and len(set(np.array(taken) // 3 // 64)) >= 2
    # the NaN twin differs from the -inf map in the planted cells only, and two of them are among the taken background
    for name in ("nan_heat_circle", "nan_heat_rotate"):
        c = EC.case(name)
        diff = np.nonzero(c["h"].view(np.int32) != c["h_nan"].view(np.int32))
        assert len(diff[0]) == 4 and np.isnan(c["h_nan"][diff]).all() and np.isneginf(c["h"][diff]).all()
        cells = (diff[1] * c["h"].shape[2] + diff[2]).tolist()
        assert cells == [0, 2, 5, 19] and {0, 2} <= {cell for cell, _ in c["expect"][0][0]}
    # every on-the-bound object of the range cases is exactly on its bound
    c = EC.case("range_coder_on")
    w = EC.expected_rows(dict(c, p=dict(c["p"], merge=False)))[0][0]["boxes"]
    on = [w[k, k % 3] for k in range(6)]
    assert on == EC.RANGE
    assert all(name in EC.NAMES for name in ("thr_falsy_none", "thr_falsy_zero", "range_limit_none", "k1_two_tasks"))
