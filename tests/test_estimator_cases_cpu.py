"""CPU checks of the generated estimator cases (tests/estimator_cases.py): that every case reaches the kernel path it exists
for.  Everything is computed from ``EN.inside`` on the case's final points (``case['hits']``, ``case['reach']``) and stated in
the kernel's constants, which are read from csrc/estimator.hip and include/al3d.h and compared with the case file's mirrors:
after a change of EST_WTILE, EST_QCAP, EST_WAVES, EST_GROUP or AL3D_EST_MAX_BOXES these tests fail until the cases reach
the new edges.  ``pytest -s`` prints the queue levels and the float32 gaps."""
import os
import re

import numpy as np
import pytest

import estimator_cases as EC
import estimator_f32 as E32
import estimator_numpy as EN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, Q = EC.T, EC.Q
LAYOUTS = [n for n in EC.NAMES if n.startswith("E_")]
VALUES = [n for n in EC.NAMES if n.startswith("F_")]
# post 8 with one task, or one frame of two, has 16 slots at most: these cannot hold 20 survivors
SMALL = ("B1", "B2", "E_nc3") + tuple(VALUES)


def survivor_total(c):
    return sum(len(v) for v in c["reach"]["survivors"].values())


def test_constants_mirror_the_kernel():
    from al3d import selector_ops as ops
    src = open(os.path.join(os.path.dirname(ops.__file__), "csrc", "estimator.hip")).read()
    define = lambda name: re.search(rf"^#define {name} (.+?)\s*(?://.*)?$", src, re.M).group(1).strip()      # noqa: E731
    assert define("EST_PPL") == "8" and define("EST_WTILE") == "(64 * EST_PPL)" and EC.T == 64 * 8
    assert int(define("EST_QCAP")) == EC.Q
    assert int(define("EST_WAVES")) == EC.WAVES
    assert int(define("EST_GROUP")) == EC.GROUP
    assert "if (cnt > EST_QCAP - EST_WTILE) drain();" in src           # the rule ``reach['levels']`` simulates
    assert src.count("+= 64) {") == 2 and EC.CHUNK == 64               # the two ballot compactions
    hdr = open(os.path.join(ROOT, "include", "al3d.h")).read()
    assert int(re.search(r"#define AL3D_EST_MAX_BOXES (\d+)", hdr).group(1)) == EC.MAX_BOXES == ops.EST_MAX_BOXES


@pytest.mark.parametrize("name", EC.NAMES)
def test_margin_holds_and_drops_little(name):
    """The builder's drop share, and the margin itself recomputed on the final points."""
    c = EC.case(name)
    print(f"{name}: {c['dropped']:.3%} of the points dropped")
    assert c["dropped"] <= 0.05 == EC.MAX_DROPPED and EC.MARGIN == 1e-3
    B, nt, post = c["labels"].shape
    assert c["boxes"].dtype == np.float32 and c["points"].dtype == np.float32 and c["offsets"].dtype == np.int64
    for b in range(B):
        lo, hi = int(c["offsets"][b]), int(c["offsets"][b + 1])
        keep = np.array([k for k in range(lo, hi) if k not in c["exempt"]], dtype=np.int64)
        if not len(keep):
            continue
        p = c["points"][keep].astype(np.float64)
        for s in c["hits"][b][0]:
            box = c["boxes"][b, s // post, s % post]
            if not (np.isfinite(box[:6]).all() and np.isfinite(box[c["rot_col"]])):
                continue
            assert EN.edge_distance(p[:, :2], EN.footprint(box, c["rot_col"])).min() >= 1e-3
            assert np.abs(np.abs(p[:, 2] - float(box[2])) - float(box[5]) / 2).min() >= 1e-3


def test_a_reaches_every_frame_and_the_one_point_tile():
    c = EC.case("A")
    r = c["reach"]
    assert c["boxes"].shape == (4, 2, 8, 9) and np.diff(c["offsets"]).tolist() == [700, 0, 513, 40]
    assert r["tiles"] == [2, 0, 2, 1] and r["frames_hit"] == [0, 2, 3]
    # five wave tiles over two workgroups; frame 2 starts at wave 2 of workgroup 0
    assert sum(r["tiles"]) == EC.WAVES + 1 and r["tiles"][0] < EC.WAVES < r["tiles"][0] + r["tiles"][2] + 1
    for b in (0, 2, 3):
        with_points = sum(len(r["survivors"][(b, t)]) for t in range(2))
        valid = int(np.clip(c["counts"][b], 0, 8).sum())
        assert with_points >= 3 and valid - with_points >= 1
    assert int(c["counts"][1].sum()) > 0 and not r["survivors"][(1, 0)] and not r["survivors"][(1, 1)]
    # the one-point tile: its point is inside exactly one valid box, and is that box's only point
    b, w = r["lone_tile"]
    slots, mask = c["hits"][b]
    assert mask.shape[1] == T + 1 and w == 1
    owners = [s for k, s in enumerate(slots) if mask[k, T]]
    assert owners == [r["lone_box"][1]] and mask[slots.index(owners[0])].sum() == 1
    assert r["levels"][(b, w)][-1] == 1
    assert any(f == 0 for f, _ in r["two_tile_boxes"])      # two waves max into one pooled row
    # slots behind the counts with points around them: they must come back 0
    behind = 0
    for b in (2, 3):
        pts = c["points"][c["offsets"][b]:c["offsets"][b + 1]]
        for t in range(2):
            for i in range(int(c["counts"][b, t]), 8):
                behind += int(EN.inside(pts, c["boxes"][b, t, i]).sum())
    assert behind > 10
    assert survivor_total(c) >= 20


def test_b_reaches_the_exact_capacity_and_the_threshold_plus_one():
    b1, b2 = EC.case("B1"), EC.case("B2")
    for c in (b1, b2):
        assert np.diff(c["offsets"]).tolist() == [2 * T + 37] and c["dropped"] == 0.0
        print(c["reach"]["levels"], c["reach"]["drains"])
    lv = b1["reach"]["levels"]
    for w in (0, 1):
        assert lv[(0, w)][:2] == [T, Q]                     # 512, then exactly EST_QCAP: queue index 1023 is written
        assert 200 < lv[(0, w)][2] < 312                    # the half box, after the drain
        assert lv[(0, w)][3] == lv[(0, w)][2] + T > Q - T   # more boxes after a drain, and a second drain
        assert b1["reach"]["drains"][(0, w)] == 2
    assert lv[(0, 2)][:2] == [37, 74] and lv[(0, 2)][3] == lv[(0, 2)][2] + 37 and b1["reach"]["drains"][(0, 2)] == 0
    assert Q in sum(lv.values(), [])
    lv = b2["reach"]["levels"]
    assert lv[(0, 0)] == [1, T + 1, T] and T + 1 == Q - T + 1 and b2["reach"]["drains"][(0, 0)] == 1
    assert lv[(0, 1)] == [0, T, Q] and lv[(0, 2)] == [0, 37, 74]
    slots, mask = b2["hits"][0]
    assert slots == [0, 1, 2] and np.nonzero(mask[0])[0].tolist() == [b2["reach"]["lone_point"]]
    # box centres inside the points' bounding square
    for c in (b1, b2):
        xy = c["points"][:, :2]
        n = int(np.clip(c["counts"][0, 0], 0, 4))
        assert (c["boxes"][0, 0, :n, :2] >= xy.min(0)).all() and (c["boxes"][0, 0, :n, :2] <= xy.max(0)).all()


def test_c_reaches_the_second_chunk_and_every_head_wave():
    c = EC.case("C")
    r = c["reach"]
    assert c["boxes"].shape[:3] == (2, 2, 160) and c["counts"].tolist() == [[160, 70], [65, 0]]
    counts = {k: len(v) for k, v in r["survivors"].items()}
    print("survivors per (frame, task):", counts)
    live = [n for (b, t), n in counts.items() if c["counts"][b, t] > 0]
    assert all(n > EC.WAVES * EC.GROUP for n in live)       # a second trip of the head's group loop, on every wave
    assert {n % EC.GROUP for n in live} >= {1, 2, 3}        # ragged last groups of every size
    assert counts[(1, 1)] == 0                              # count 0: 160 populated boxes, none tested
    for lo in (EC.CHUNK, 2 * EC.CHUNK):                     # rows move (src != dst) in the second and third chunk
        kept = [i for i in r["survivors"][(0, 0)] if i >= lo]
        empty = [i for i in range(lo, 160) if i not in r["survivors"][(0, 0)]]
        assert kept and empty and min(empty) < max(kept)
        assert all(r["survivors"][(0, 0)].index(i) != i for i in kept)
    assert [i for i in r["survivors"][(0, 1)] if i >= EC.CHUNK] and [i for i in range(64, 70) if i not in r["survivors"][(0, 1)]]
    assert all(n > EC.CHUNK for n in (c["counts"][0, 0], c["counts"][0, 1], c["counts"][1, 0]))
    # in the footprint, above the height: some empty valid boxes have points over them
    over = 0
    for b in range(2):
        pts = c["points"][c["offsets"][b]:c["offsets"][b + 1]].astype(np.float64)
        for t in range(2):
            for i in range(int(c["counts"][b, t])):
                if i not in r["survivors"][(b, t)]:
                    box = c["boxes"][b, t, i]
                    over += int((EN.edge_cross(pts[:, :2], EN.footprint(box)) > 0).all(axis=1).sum())
    assert over >= 20
    sizes, ang = c["boxes"][..., 3:5], c["boxes"][..., 6]
    assert sizes.min() >= 0.5 and sizes.max() <= 2.5 and ang.min() < -np.pi and ang.max() > np.pi


def test_d_fills_the_table():
    c = EC.case("D")
    r = c["reach"]
    assert c["boxes"].shape == (1, 1, EC.MAX_BOXES, 9) and int(c["counts"][0, 0]) == EC.MAX_BOXES
    assert r["survivors"][(0, 0)] == list(range(EC.MAX_BOXES))
    slots, mask = c["hits"][0]
    assert mask.any(axis=0).all() and c["dropped"] == 0.0   # every point is inside a box
    assert 2000 <= mask.shape[1] <= 3000
    assert any(mask[EC.MAX_BOXES - 1, w * T:(w + 1) * T].any() for w in range(r["tiles"][0]))     # box index 1023 is queued


@pytest.mark.parametrize("name", LAYOUTS)
def test_e_layouts(name):
    c = EC.case(name)
    r = c["reach"]
    B, nt, post, D = c["boxes"].shape
    want = dict(E_dim7=(7, 6, 5, (4, 6)), E_dim11_rot8=(11, 8, 5, (4, 6)), E_f3=(9, 6, 3, (4, 6)), E_f6=(9, 6, 6, (4, 6)),
                E_nc3=(9, 6, 5, (3,)), E_nc32=(9, 6, 5, (10, 10, 12)), E_tail=(9, 6, 5, (4, 6)))[name]
    assert (D, c["rot_col"], c["points"].shape[1], c["classes"]) == want
    assert (B, post) == (2, 8) and nt == len(c["classes"]) and c["num_classes"] == sum(c["classes"])
    assert r["tiles"] == [2, 1] and r["frames_hit"] == [0, 1]
    labels = [int(c["labels"][b, t, i]) for (b, t), keep in r["survivors"].items() for i in keep]
    assert 0 in labels and c["num_classes"] - 1 in labels   # the first and the last one-hot column
    lo = np.concatenate([[0], np.cumsum(c["classes"])])
    for t in range(nt):
        assert (c["labels"][:, t] >= lo[t]).all() and (c["labels"][:, t] < lo[t + 1]).all()
    for b in range(2):
        with_points = sum(len(r["survivors"][(b, t)]) for t in range(nt))
        assert with_points >= 3 and int(c["counts"][b].sum()) - with_points >= 1
    assert len(c["points"]) - int(c["offsets"][-1]) == (100 if name == "E_tail" else 0)
    if name == "E_tail":                                    # the rows behind the last offset would be hits in frame 0
        assert EN.inside(c["points"][c["offsets"][-1]:], c["boxes"][0, 0, 0]).any()
    if name == "E_dim11_rot8":                              # column 6 is junk there: it gives other memberships
        slots, mask = c["hits"][0]
        other = np.stack([EN.inside(c["points"][:c["offsets"][1]], c["boxes"][0, s // 8, s % 8], 6) for s in slots])
        assert (other != mask).sum() > 50
    if name not in SMALL:
        assert survivor_total(c) >= 20


@pytest.mark.parametrize("name", VALUES)
def test_f_values(name):
    c = EC.case(name)
    r = c["reach"]
    clean = EC.case("F_clean")
    slots, mask = c["hits"][0]
    assert c["boxes"].shape == (1, 2, 8, 9) and r["tiles"] == [2]
    # the exact-boundary memberships, in float64 on the float32 values; the kernel's float32 products are exact there too
    assert np.array_equal(c["boxes"][0, 1, 7], EC.EDGE_BOX)
    pts = c["points"][r["edge_points"]]
    assert [tuple(float(v) for v in p[:3]) for p in pts] == [tuple(float(np.float32(v)) for v in xyz) for xyz, _ in EC.EDGE_POINTS]
    assert EN.inside(pts, EC.EDGE_BOX).tolist() == [w for _, w in EC.EDGE_POINTS]
    assert pts[3, 0] == 65.0 and 65.0 - float(pts[4, 0]) == 2.0 ** -17        # one float32 ulp inside the edge
    if name != "F_counts":
        assert mask[slots.index(r["edge_slot"])].sum() == sum(w for _, w in EC.EDGE_POINTS)
    # slots (0, 5..7) drop out in every variant; the other slots hold the clean case's points
    for s in r["dirty_slots"]:
        assert mask[slots.index(s)].sum() == 0
    same = [k for k in range(len(c["points"])) if k not in r["bad_points"]]
    assert np.array_equal(c["points"][same].view(np.int32), clean["points"][same].view(np.int32))
    cs, cm = clean["hits"][0]
    for k, s in enumerate(slots):
        if s not in r["dirty_slots"]:
            assert np.array_equal(mask[k], cm[cs.index(s)])
    if name == "F_clean":
        near = np.abs(c["boxes"][0, 0, 5:8, None, 0] - c["points"][None, :, 0]).min()
        assert near >= 200.0 and np.isfinite(c["boxes"]).all() and np.isfinite(c["points"]).all()
    if name == "F_dirty1":
        d = c["boxes"][0, 0, 5:8]
        assert np.isnan(d[0, 0]) and np.isnan(d[1, 6]) and d[2, 3] == 0.0
        bad = c["points"][r["bad_points"], :3]
        assert np.isnan(bad[0, 0]) and bad[1, 0] == np.inf and bad[2, 2] == -np.inf
    if name == "F_dirty2":
        d = c["boxes"][0, 0, 5:8]
        assert d[0, 3] == -1.5 and np.isnan(d[1, 3]) and d[2, 5] == -1.0
    if name in ("F_dirty1", "F_dirty2"):
        base = c["boxes"][0, 0, 0]
        others = np.delete(np.arange(9), [0, 3, 5, 6])
        assert mask[slots.index(0)].sum() >= 20                # they sit on a populated box
        assert all(np.array_equal(d[k, others], base[others]) for k in range(3))
        for p in c["points"][r["bad_points"], :3]:          # the finite coordinates are the populated box's centre
            ok = np.isfinite(p)
            assert np.array_equal(p[ok], base[:3][ok])
    if name == "F_counts":
        y = E32.yardstick(name)
        assert c["counts"].tolist() == [[13, -3]]
        assert slots == list(range(8))                      # post + 5 clamps to post, -3 to 0
        assert y["counts"].tolist() == [[len(r["survivors"][(0, 0)]), 0]] and (y["npts"][0, 1] == 0).all()
        assert np.array_equal(y["npts"][0, 0], E32.yardstick("F_clean")["npts"][0, 0])


@pytest.mark.parametrize("name", EC.NAMES)
def test_yardstick_agrees_with_reach_and_the_f32_gap_is_usable(name):
    c = EC.case(name)
    y = E32.yardstick(name)
    B, nt, post = c["labels"].shape
    for b in range(B):
        slots, mask = c["hits"][b]
        want = np.zeros(nt * post, dtype=np.int64)
        want[slots] = mask.sum(1)
        assert np.array_equal(y["npts"][b].ravel(), want)
    assert y["survivors"] == [c["reach"]["survivors"][(b, t)] for b in range(B) for t in range(nt)]
    n = survivor_total(c)
    print(f"{name}: {n} survivors; float32 torch against float64: IoU {y['e32_iou']:.3e}, pooled {y['e32_pooled']:.3e} "
          f"(max |pooled| {np.abs(y['pooled']).max():.2f})")
    assert n == len(y["owners"]) and (n >= 20 or name in SMALL)
    assert np.isfinite(y["e32_iou"]) and 0 < y["e32_iou"] < 1e-5
    assert np.isfinite(y["e32_pooled"]) and 0 < y["e32_pooled"] < 1e-3
    assert np.isfinite(y["iou"][~np.isnan(y["f32_iou"])]).all()
