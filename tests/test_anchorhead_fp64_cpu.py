"""CPU suite of the anchor head's float64 yardstick (tests/head_fp64.py) and of the planted cases (tests/anchorhead_cases.py):
the yardstick against the reference's own ``predict`` golden, the measured float32 band, the conditions the plants promise,
the float32 oracle's sequential rule on every case, and the demonstrations that the GPU comparison bites."""
import os

import numpy as np
import pytest

import anchorhead_cases as AC
import head_fp64 as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_predict_tasks.npz")
RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]


def test_yardstick_equals_the_reference_predict_golden():
    """``MultiGroupHead.predict`` of the reference (mg_head.py:697-803) on seeded head outputs of a 16 x 16 map, as
    test_head_predict_golden.py pins the oracle: same detections in the same order, scores to one float32 ulp, boxes to the
    golden's float32 precision."""
    z = np.load(GOLD)
    B, Hh, W = (int(v) for v in z["shape"])
    ncs = [int(v) for v in z["num_classes"]]
    off = np.concatenate([[0], np.cumsum(ncs)])
    for b in range(B):
        bb, ss, ll = [], [], []
        for t, nc in enumerate(ncs):
            na = 2 * nc
            hout = np.concatenate([z[f"box{t}"][b].reshape(Hh * W, -1), z[f"cls{t}"][b].reshape(Hh * W, -1)], axis=1)
            r = H.task_predict(hout, z[f"anchors{t}"], na, nc, 0, na * 10, AC.SCORE_THR, AC.THR, 1000, 83, RANGE)
            bb.append(r["boxes"]); ss.append(r["scores"]); ll.append(r["labels"] + off[t])
        bb, ss, ll = np.concatenate(bb), np.concatenate(ss), np.concatenate(ll)
        rb, rs, rl = z[f"out{b}.boxes"], z[f"out{b}.scores"], z[f"out{b}.labels"]
        assert ll.tolist() == rl.tolist() and len(rl) > 300
        assert np.all(np.abs(ss - rs) <= 1.2e-7 * np.maximum(np.abs(rs), 1e-3))
        np.testing.assert_allclose(bb[:, :8], rb[:, :8], rtol=2e-6, atol=2e-6)
        d = np.abs(bb[:, 8] - rb[:, 8])
        assert np.minimum(d, 2 * np.pi - d).max() < 1e-5
    assert not np.any(z["out1.labels"] == off[3])


def test_measured_band_is_within_the_recorded_one(oracle):
    """Recompute max |IoU_f32 - IoU_f64| per placement and footprint over the pairs of every family: none exceeds the figure
    recorded in anchorhead_cases.MEASURED nor falls below 0.8 of it (the figures are re-recorded when the plants move), and
    delta at range stays under the kernel's 0.1 % prefilter margin."""
    got = AC.measure_band(oracle)
    for placement, m in got.items():
        print(placement, {f: f"{v:.2e}" for f, v in m.items()}, "delta", AC.DELTA[placement])
        assert set(m) == set(AC.MEASURED[placement])
        for f, v in m.items():
            assert 0.8 * AC.MEASURED[placement][f] <= v <= AC.MEASURED[placement][f], (placement, f, v)
        assert max(v for f, v in m.items() if f != "other") <= AC.TIGHT_MAX[placement]
    assert AC.DELTA["origin"] < AC.DELTA["range"] < 1e-3 * AC.THR and AC.DELTA_TIGHT["range"] <= AC.DELTA["range"]


@pytest.mark.parametrize("family,placement", AC.CASES)
def test_cases_stay_off_the_thresholds_and_the_oracle_agrees(oracle, family, placement):
    """No evaluated pair within delta of the IoU threshold (tight_bounds' +-2 delta plants sit at 2 delta; the one exact
    on-threshold plant of degenerate/origin is exempt), no score within 1e-3 of the score threshold except the planted ones,
    no centre within 1e-4 of a range bound; the float32 oracle's sequential NMS on the float64-decoded boxes keeps the
    yardstick's set in every (sample, task); random_at_range redrew under 1 % and has >= 300 overlapping pairs per task."""
    case, ref, pairs = AC.make(family, placement)
    delta, p = (AC.DELTA_TIGHT if family == "tight_bounds" else AC.DELTA)[placement], case["params"]
    exempt = set()
    if family == "degenerate" and placement == "origin":
        exempt = {tuple(case["expect"][t]["on_threshold"]) + (t,) for t in case["expect"]}
    for (b, t), pl in pairs.items():
        cand = ref[b][t]["cand"]
        for i, j, q in pl:
            if (int(cand[i]), int(cand[j]), t) in exempt:
                assert q["iou"] == AC.THR
                continue
            gap = abs(q["iou"] - AC.THR)
            assert gap >= (1.5 * delta if family == "tight_bounds" else delta), (b, t, i, j, q["iou"])
    rng = np.asarray(p["rng"], np.float64).reshape(2, 3)
    marks = case.get("marks", {})
    for b, row in enumerate(ref):
        for t, r in enumerate(row):
            cb = r["cand_boxes"]
            xyz = cb[:, :3][np.isfinite(cb[:, :3]).all(1)]
            assert not (np.abs(xyz[:, None, :] - rng[None]) < 1e-4).any()
            s = H.sigmoid(case["hout"][b][:, case["cls_off"][t]:case["cls_off"][t] + case["na"][t] * case["nc"][t]]).reshape(-1)
            near = np.abs(s.reshape(-1, case["nc"][t]).max(1) - p["score_thresh"]) < 1e-3
            assert near.sum() == (2 if (t == 2 and marks) else 0)
            keep32 = oracle.rotate_nms(cb[:, [0, 1, 3, 4, 8]].astype(np.float32), p["iou_thresh"], p["post_max"])
            assert keep32.tolist() == r["nms_keep"].tolist(), (b, t)
    if family == "random_at_range":
        assert case["redrawn_share"] < 0.01
        assert min(case["overlapping_pairs"].values()) >= 300
        print("redrawn share", case["redrawn_share"], case["overlapping_pairs"])


@pytest.mark.parametrize("placement", list(AC.PLACEMENTS))
def test_tight_bounds_pairs_are_what_was_planted(placement):
    """The pair collector on every plant: the bound the pair was built on EQUALS the float64 IoU (1e-12; for the axis-aligned
    boxes at +-pi/2 and pi 2e-6, because float32(pi/2) is not pi/2 and the box is turned by 4e-8 .. 9e-8 rad against its
    stand-up box: 1.3e-6 for the 6 m sliver), the IoU sits at thr * (1 + eps) up to the float32 rounding of the planted coordinates (half of delta: two centres
    rounded by 1.9e-6 m at 48 m move the 0.3 m sliver's IoU by 7e-6; the band plants stay 1.5 delta off the threshold), the
    later box falls exactly when eps > 0, and no pair meets anything but its partner."""
    case, ref, pairs = AC.make("tight_bounds", placement)
    delta = AC.DELTA_TIGHT[placement]
    eps_seen = set()
    for (b, t), plants in case["plants"].items():
        kind, r, _ = AC.TIGHT_KINDS[t]
        cand = ref[b][t]["cand"].tolist()
        by_anchor = {frozenset((cand[i], cand[j])): q for i, j, q in pairs[(b, t)]}
        assert len(by_anchor) == len(plants) == len(pairs[(b, t)])
        for i, j, ep, _, foot in plants:
            q = by_anchor[frozenset((i, j))]
            bound = {"nested": q["ratio"], "axis": q["standup"], "par": min(q["own_a"], q["own_b"])}[kind]
            assert abs(bound - q["iou"]) <= (1e-12 if kind != "axis" or r == 0.0 else 2e-6), (kind, r, foot, bound - q["iou"])
            assert max(q["own_a"], q["own_b"]) - q["iou"] <= 1e-6 and q["ratio"] >= q["iou"] - 1e-12 and q["standup"] >= q["iou"] - 1e-12
            assert abs(q["iou"] - AC.THR * (1.0 + ep)) <= 0.5 * delta, (kind, foot, ep, q["iou"])
            later = j if cand.index(i) < cand.index(j) else i
            assert (later not in ref[b][t]["anchors"].tolist()) == (ep > 0)
            eps_seen.add(ep)
    assert eps_seen == set(AC.eps_list(placement)) and 2 * delta / AC.THR in eps_seen
    inside = [e for e in eps_seen if 0 < e < 1e-3]                        # plants inside the 0.1 % margin, at both placements
    assert len(inside) >= 2 and {7e-4, -7e-4, 1.5e-3, -1.5e-3, 1e-2, -1e-2} <= eps_seen
    if placement == "origin":
        assert {3e-4, -3e-4} <= eps_seen


@pytest.mark.parametrize("placement", list(AC.PLACEMENTS))
def test_planted_outcomes(placement):
    """What the builders promise, on the yardstick: degenerate pairs fall or stand as listed, a NaN box is kept by the NMS and
    suppresses nothing, and only a NaN centre (NaN x, or a NaN width through the anchor's diagonal) fails the range mask; in a chain ranked along its rows every other box survives and a
    clique leaves one; the pre_max / post_max / tie / threshold plants of cuts."""
    case, ref, _ = AC.make("degenerate", placement)
    for t, e in case["expect"].items():
        for b in range(2):
            assert sorted(ref[b][t]["anchors"].tolist()) == sorted(set(e["kept"]) - set(e["nan_centre"])), (b, t)
            assert set(e["nan_centre"]) <= set(ref[b][t]["cand"][ref[b][t]["nms_keep"]].tolist())      # kept by the NMS
            assert e["nan_angle"] in ref[b][t]["anchors"]
        assert len(e["suppressed"]) == (7 if placement == "origin" else 6)
    case, ref, _ = AC.make("chains", placement)
    rows, clique = case["rows"][0]
    want = [k for row in rows for k in row[::2]] + clique[:1]
    assert ref[0][0]["anchors"].tolist() == want
    for b in range(2):
        for t in range(4):
            got = set(ref[b][t]["anchors"].tolist())
            assert len(got & set(case["rows"][t][1])) == 1
            assert len(got) >= 1 + sum(-(-n // 2) for n in AC.CHAIN_LENGTHS) - 6       # a chain entered mid-way loses at most one
    for pre, post in ((1000, 83), (1024, 128)):
        case, ref, _ = AC.make(f"cuts_{pre}_{post}", placement)
        r = ref[0]
        m = case["marks"]
        assert len(r[0]["cand"]) == len(r[1]["cand"]) == pre and len(r[0]["nms_keep"]) == post
        assert 0 < len(r[0]["anchors"]) < post                                  # the range mask removed survivors
        for t in (0, 1):                                                         # the run of equal scores: lowest anchors go in
            run = np.sort(m["tie_run"][t])
            took = sorted(set(r[t]["cand"].tolist()) & set(run.tolist()))
            assert took == run[:pre - 989].tolist() and 0 < len(took) < 50
        assert len(r[1]["nms_keep"]) == 30 + (pre - 989)                        # one per clique + every admitted separate box
        assert m["at"] in r[2]["anchors"] and m["below"] not in r[2]["cand"]
        assert len(r[2]["cand"]) == 13 and len(r[2]["nms_keep"]) == 10 and len(r[2]["anchors"]) == 4
        assert len(r[3]["cand"]) == 0 and len(r[4]["anchors"]) == 1


def test_the_comparison_bites():
    """Host-side demonstrations on the yardstick's own output in the library's format: dropping one survivor fails the
    comparison; flipping one +-3e-4 tight_bounds decision fails it; the wrong rule ``>`` changes the expected set of the
    on-threshold plant (and of nothing else in that case)."""
    def as_library(case, ref, sentinel=-7777.0):
        B, nt, post = len(ref), len(ref[0]), case["params"]["post_max"]
        boxes = np.full((B, nt, post, 9), sentinel, np.float32)
        scores = np.full((B, nt, post), sentinel, np.float32)
        labels = np.full((B, nt, post), int(sentinel), np.int32)
        counts = np.zeros((B, nt), np.int32)
        for b, row in enumerate(ref):
            for t, r in enumerate(row):
                k = len(r["anchors"])
                boxes[b, t, :k], scores[b, t, :k], labels[b, t, :k] = r["boxes"], r["scores"], r["labels"] + case["label_off"][t]
                counts[b, t] = k
        return boxes, scores, labels, counts

    def drop(got, b, t, pos, sentinel=-7777.0):
        boxes, scores, labels, counts = (a.copy() for a in got)
        k = counts[b, t]
        for a in (boxes, scores, labels):
            a[b, t, pos:k - 1] = a[b, t, pos + 1:k]
            a[b, t, k - 1] = sentinel
        counts[b, t] = k - 1
        return boxes, scores, labels, counts

    case, ref, _ = AC.make("chains", "range")
    good = as_library(case, ref)
    AC.compare(case, ref, good)
    with pytest.raises(AssertionError):
        AC.compare(case, ref, drop(good, 1, 2, 5))
    case, ref, _ = AC.make("tight_bounds", "origin")
    good = as_library(case, ref)
    AC.compare(case, ref, good)
    flipped = 0
    for (b, t), plants in case["plants"].items():
        for i, j, ep, kind, foot in plants:
            if ep == -3e-4 and not flipped:                                     # both stand; a wrong kernel suppresses the later one
                pos = max(ref[b][t]["anchors"].tolist().index(i), ref[b][t]["anchors"].tolist().index(j))
                with pytest.raises(AssertionError):
                    AC.compare(case, ref, drop(good, b, t, pos))
                flipped += 1
    assert flipped == 1
    case, ref, _ = AC.make("degenerate", "origin")
    wrong = AC.expected(case, strict=True)
    for t, e in case["expect"].items():
        for b in range(2):
            extra = set(wrong[b][t]["anchors"].tolist()) - set(ref[b][t]["anchors"].tolist())
            assert extra == {e["on_threshold"][1]}
