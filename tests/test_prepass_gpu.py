"""GPU suite for the PPAL / CALD pre-passes: ``selector_ops.match_boxes`` (csrc/box_match.hip) against the reference's own
``accumulate`` (tests/golden/prepass_match.npz, tools/gen_golden_prepass.py) and, at the edge cases, against its float64
restatement tests/prepass_numpy.py (which tests/test_prepass_host.py pins to the same golden); the augmented view; the
loaders' ``view`` argument; ``CaldSelector(prepass=True)`` end to end.

Tolerances (u = 2^-24, the float32 unit roundoff; the references are float64):

* ``match_ref``, ``cls_count``: equal.  Every coordinate of the fixtures is a multiple of 1/64 below 64, so every centre
  difference is exact in float32, squared distances below 16 are exact, no distance lies within 1e-4 of ``dist_th`` and
  candidate distances are 1e-4 apart or exactly tied.
* ``match_iou``: rtol 64 u.  inter = three minima (exact) and two products (2 u); each volume two products (2 u); the union
  is vol_a + vol_b - inter: two sums (2 u) of terms carrying 2 u each, and since inter <= min(vol_a, vol_b) the union is at
  least max(vol_a, vol_b), so its absolute error is at most about (2 + 2) u (vol_a + vol_b) + 3 u inter <= ~ 15 u union;
  the quotient adds 1 u: about 2 + 15 + 1 + the inputs' own conversion = 21 u.  A view adds one division per size (3 u on
  each product) and the sizes' own rounding when they were scaled (3 u more): 64 u leaves room for both.
* ``cls_quality``: rtol (n_c + 16) u * 2 per class: each term is pow(s, 0.6) * pow(iou, 0.4) (two pow calls of a few u, the
  iou's 21 u enters with exponent 0.4, one product), all terms positive, and n_c sequential additions add at most n_c u.
* ``cls_cons``: atol 5e-6: |iou + 0.5 (p + q) - 1.3| with every term below 2.3, i.e. a handful of roundings of 1.2e-7 each
  plus the iou's 21 u and the float32 value of 1.3 (4.8e-8 off).
"""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import prepass_numpy as PN

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
NCLS = 10
E2E_BUDGET = 12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "prepass_match.npz"), allow_pickle=False)


def run_kernel(dev, boxes, scores, labels, counts, ref_boxes, ref_labels, ref_scores, ref_off, **kw):
    from al3d import selector_ops as ops
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a, dtype=d)).to(dev)      # noqa: E731
    for k in ("class_range", "origin"):
        if kw.get(k) is not None:
            kw[k] = t(kw[k], np.float32)
    out = ops.match_boxes(t(boxes, np.float32), t(scores, np.float32), t(labels, np.int32), t(counts, np.int32),
                          t(np.asarray(ref_boxes, np.float32).reshape(len(ref_labels), 9), np.float32),
                          t(ref_labels, np.int32), t(ref_scores, np.float32), t(ref_off, np.int32), NCLS, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(got, want, label=""):
    """``want``: float64 arrays of the reference or its restatement.  Every frame, slot and class is compared."""
    assert np.array_equal(got["match_ref"], want["match_ref"]), label
    assert np.array_equal(got["cls_count"], want["cls_count"]), label
    iou_err = np.abs(got["match_iou"] - want["match_iou"])
    print(label, "matches", int(want["cls_count"].sum()), "max iou rel err / u",
          float((iou_err / np.maximum(want["match_iou"], 1e-30)).max() / U),
          "max quality rel err / u", float((np.abs(got["cls_quality"] - want["cls_quality"])
                                            / np.maximum(want["cls_quality"], 1e-30)).max() / U),
          "max cons abs err", float(np.abs(got["cls_cons"] - want["cls_cons"]).max()))
    assert np.all(iou_err <= 64 * U * want["match_iou"]), label
    assert np.all(got["match_iou"][want["match_ref"] < 0] == 0)
    n_c = want["cls_count"].astype(np.float64)
    assert np.all(np.abs(got["cls_quality"] - want["cls_quality"]) <= (n_c + 16) * 2 * U * want["cls_quality"]), label
    assert np.all(np.abs(got["cls_cons"] - want["cls_cons"]) <= 5e-6), label
    assert np.all(got["cls_cons"][want["cls_count"] == 0] == 1.0) and np.all(got["cls_quality"][want["cls_count"] == 0] == 0)


def golden_inputs(z):
    return [z[k] for k in ("boxes", "scores", "labels", "counts", "ref_boxes", "ref_labels", "ref_scores", "ref_off")]


def test_golden_reference_accumulate(dev, z):
    got = run_kernel(dev, *golden_inputs(z), dist_th=float(z["dist_th"]))
    want = {k: z[k] for k in ("match_ref", "match_iou", "cls_count", "cls_quality", "cls_cons")}
    assert want["cls_count"].sum() > 60
    check(got, want, "golden")


# ------------------------------------------------------------------------------------------------ edge cases
def box(x, y, w=2.0, l=4.0, h=1.5):
    return [x, y, 0.0, w, l, h, 0.0, 0.0, 0.0]


def pack(frames, nt=1, post=None):
    """``frames``: per frame a list per task of (box, score, label) -> the raw NMS layout; unused slots hold junk."""
    post = post or max([1] + [len(t) for f in frames for t in f])
    B = len(frames)
    boxes = np.full((B, nt, post, 9), 3.0, np.float32)
    scores = np.full((B, nt, post), 0.999, np.float32)
    labels = np.zeros((B, nt, post), np.int32)
    counts = np.zeros((B, nt), np.int32)
    for b, f in enumerate(frames):
        for t, task in enumerate(f):
            counts[b, t] = len(task)
            for i, (bx, s, lab) in enumerate(task):
                boxes[b, t, i], scores[b, t, i], labels[b, t, i] = bx, s, lab
    return boxes, scores, labels, counts


def refs_of(frames):
    """``frames``: per frame a list of (box, label, score)."""
    rows = [r for f in frames for r in f]
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int32)
    return (np.array([r[0] for r in rows], np.float32).reshape(len(rows), 9), np.array([r[1] for r in rows], np.int32),
            np.array([r[2] for r in rows], np.float32), off)


def grid(rng, lo, hi, size=None):
    return (rng.integers(int(lo * 64), int(hi * 64), size=size) / 64.0).astype(np.float32)


def crowd(rng, npred, nref, cls, nt=2, post=None, equal_scores=True):
    """One frame with ``npred`` predictions and ``nref`` references of class ``cls`` in a 24 m square (many candidates per
    prediction, references get taken), under the fixture conditions: a prediction with a candidate within 1e-4 of the
    threshold or two candidates closer than 1e-4 without being exactly tied is drawn again."""
    rb = np.zeros((nref, 9), np.float32)
    rb[:, 0], rb[:, 1], rb[:, 3:6] = grid(rng, -12, 12, nref), grid(rng, -12, 12, nref), grid(rng, 0.5, 5, (nref, 3))
    preds = []
    while len(preds) < npred:
        p = np.zeros(9, np.float32)
        anchor = rb[rng.integers(0, nref)]
        p[:2] = anchor[:2] + grid(rng, -1.5, 1.5, 2)
        p[3:6] = grid(rng, 0.5, 5, 3)
        d = np.sort(np.linalg.norm(rb[:, :2].astype(np.float64) - p[:2].astype(np.float64), axis=1))
        gaps = np.diff(d[d < 4.0])
        if np.any(np.abs(d - 1.0) <= 1e-4) or np.any((gaps != 0) & (gaps <= 1e-4)):
            continue
        s = np.float32(rng.choice([0.25, 0.5])) if equal_scores and rng.random() < 0.3 else np.float32(rng.uniform(0.1, 0.99))
        preds.append((p, s, cls))
    per = (npred + nt - 1) // nt
    tasks = [preds[t * per:(t + 1) * per] for t in range(nt)]
    refs = [(rb[r], cls, np.float32(rng.uniform(0.1, 0.9))) for r in range(nref)]
    return tasks, refs, post or per


def case_equal_scores():
    """Two predictions with one score beside one reference: the later position goes first and takes it."""
    return pack([[[(box(10.25, 0), 0.5, 3), (box(10.5, 0), 0.5, 3)]]]), refs_of([[(box(10, 0), 3, 0.7)]]), {}


def case_equal_scores_across_tasks():
    return (pack([[[(box(10.25, 0), 0.5, 3)], [(box(10.5, 0), 0.5, 3)]]], nt=2), refs_of([[(box(10, 0), 3, 0.7)]]), {})


def case_equal_distances():
    """References at exactly 0.5 on both sides: the earlier row wins, the later one stays free for the next prediction."""
    return (pack([[[(box(0, 5), 0.9, 1), (box(0, 5.25), 0.4, 1)]]]),
            refs_of([[(box(0.5, 5), 1, 0.3), (box(-0.5, 5), 1, 0.6)]]), {})


def case_other_class_nearer():
    return (pack([[[(box(0, 0), 0.9, 2)]]]), refs_of([[(box(0.125, 0), 4, 0.5), (box(0.75, 0), 2, 0.5)]]), {})


def case_nearest_taken_second_matches():
    return (pack([[[(box(0, 0), 0.9, 0), (box(0.25, 0), 0.8, 0)]]]),
            refs_of([[(box(0.125, 0), 0, 0.5), (box(1.0, 0), 0, 0.5)]]), {})


def case_nearest_taken_nothing_left():
    return (pack([[[(box(0, 0), 0.9, 0), (box(0.25, 0), 0.8, 0)]]]),
            refs_of([[(box(0.125, 0), 0, 0.5), (box(1.5, 0), 0, 0.5)]]), {})


def case_frame_without_predictions():
    return (pack([[[]], [[(box(1, 1), 0.6, 5)]]]), refs_of([[(box(1, 1), 5, 0.2)], [(box(1, 1.5), 5, 0.2)]]), {})


def case_frame_without_references():
    return (pack([[[(box(1, 1), 0.6, 5)]], [[(box(1, 1), 0.6, 5)]]]), refs_of([[], [(box(1, 1.5), 5, 0.2)]]), {})


def case_no_reference_at_all():
    return (pack([[[(box(1, 1), 0.6, 5)]]]), refs_of([[]]), {})


def case_class_over_64_predictions():
    rng = np.random.default_rng(1)
    tasks, refs, post = crowd(rng, 150, 40, 7)
    return pack([tasks], nt=2, post=post + 3), refs_of([refs]), {}


def case_class_over_64_references():
    rng = np.random.default_rng(2)
    tasks, refs, post = crowd(rng, 50, 200, 9)
    return pack([tasks], nt=2, post=post + 1), refs_of([refs]), {}


def case_counts_equal_post():
    rng = np.random.default_rng(3)
    tasks, refs, post = crowd(rng, 66, 30, 0, nt=2)
    assert all(len(t) == post for t in tasks)
    return pack([tasks], nt=2, post=post), refs_of([refs]), {}


def case_label_outside_the_classes():
    """Labels -1 and 10 on both sides sit exactly on each other and never match; the valid pair beside them does."""
    return (pack([[[(box(0, 0), 0.9, -1), (box(5, 0), 0.9, NCLS), (box(9, 0), 0.9, 9)]]]),
            refs_of([[(box(0, 0), -1, 0.5), (box(5, 0), NCLS, 0.5), (box(9, 0.5), 9, 0.5)]]), {})


def case_class_range_each_side():
    """Range 30 from origin (1, 0) for class 8: a prediction outside it (its reference inside), a reference outside it (its
    prediction inside), a reference exactly on it (>= cuts it), and a pair inside that matches."""
    rng_ = np.full((NCLS,), 50.0, np.float32)
    rng_[8] = 30.0
    return (pack([[[(box(31.25, 0), 0.9, 8), (box(-28.75, 0), 0.8, 8), (box(1, 29.75), 0.7, 8), (box(11, 0), 0.6, 8)]]]),
            refs_of([[(box(30.75, 0), 8, 0.5), (box(-29.25, 0), 8, 0.5), (box(1, 30), 8, 0.5), (box(11, 0.5), 8, 0.5)]]),
            dict(class_range=rng_, origin=np.array([[1.0, 0.0]], np.float32)))


CASES = [case_equal_scores, case_equal_scores_across_tasks, case_equal_distances, case_other_class_nearer,
         case_nearest_taken_second_matches, case_nearest_taken_nothing_left, case_frame_without_predictions,
         case_frame_without_references, case_no_reference_at_all, case_class_over_64_predictions,
         case_class_over_64_references, case_counts_equal_post, case_label_outside_the_classes,
         case_class_range_each_side]
# what each hand-made case must show, so that a restatement sharing a mistake with the kernel cannot pass it:
# match_ref at the listed (frame, task, slot)
EXPECT = {
    "case_equal_scores": {(0, 0, 0): -1, (0, 0, 1): 0},
    "case_equal_scores_across_tasks": {(0, 0, 0): -1, (0, 1, 0): 0},
    "case_equal_distances": {(0, 0, 0): 0, (0, 0, 1): 1},
    "case_other_class_nearer": {(0, 0, 0): 1},
    "case_nearest_taken_second_matches": {(0, 0, 0): 0, (0, 0, 1): 1},
    "case_nearest_taken_nothing_left": {(0, 0, 0): 0, (0, 0, 1): -1},
    "case_frame_without_predictions": {(1, 0, 0): 1},
    "case_frame_without_references": {(0, 0, 0): -1, (1, 0, 0): 0},
    "case_no_reference_at_all": {(0, 0, 0): -1},
    "case_label_outside_the_classes": {(0, 0, 0): -1, (0, 0, 1): -1, (0, 0, 2): 2},
    "case_class_range_each_side": {(0, 0, 0): -1, (0, 0, 1): -1, (0, 0, 2): -1, (0, 0, 3): 3},
}


@pytest.mark.parametrize("case", CASES, ids=[c.__name__[5:] for c in CASES])
def test_edge_case(dev, case):
    preds, refs, kw = case()
    want = PN.match_frames(*preds, *refs, NCLS, **kw)
    for at, row in EXPECT.get(case.__name__, {}).items():
        assert want["match_ref"][at] == row, (at, row)
    if "over_64" in case.__name__ or "equal_post" in case.__name__:          # matches and misses, references get taken
        assert want["cls_count"].sum() >= 15 and (want["match_ref"][0, 0, :preds[3][0, 0]] < 0).sum() >= 5
    got = run_kernel(dev, *preds, *refs, **kw)
    check(got, want, case.__name__)


def test_more_than_max_boxes_raises(dev):
    from al3d.lib import Al3dError
    one = [(box(i, 0), 0.5, 0) for i in range(6)]
    preds, refs = pack([[one[:3], one[3:]], [one[:2], one[:3]]], nt=2), refs_of([[(box(0, 0), 0, 0.5)], []])
    run_kernel(dev, *preds, *refs, max_boxes=6)
    with pytest.raises(AssertionError, match="Only <= 5 boxes per sample allowed"):
        run_kernel(dev, *preds, *refs, max_boxes=5)
    with pytest.raises(Al3dError):                       # ref_off beyond the rows
        run_kernel(dev, *preds, refs[0], refs[1], refs[2], np.array([0, 1, 2], np.int32))


# ------------------------------------------------------------------------------------------------ the view
VIEWS = [(True, False, 0.0, 1.0), (False, True, 0.3, 0.95), (True, True, -2.5, 1.0625)]


@pytest.mark.parametrize("view", VIEWS, ids=["flip_x", "flip_y_rot_scale", "all"])
def test_points_view_against_torch(dev, view):
    """The same three steps in torch float32 (cos / sin rounded to float32 like the kernel's).  Each side is within
    4 u (|x| + |y|) |scale| of the exact result -- two products and a sum for the rotation, one product for the scaling --
    so the two differ by at most twice that; z by one product's 1 u on each side."""
    from al3d import selector_ops as ops
    g = torch.Generator().manual_seed(5)
    for P, F in ((1, 3), (1000, 5), (70001, 4)):
        pts = (torch.randn(P, F, generator=g) * 30).to(dev)
        fx, fy, rot, scale = view
        x = pts[:, 0] * (-1.0 if fy else 1.0)
        y = pts[:, 1] * (-1.0 if fx else 1.0)
        c = float(np.float32(np.cos(np.float64(np.float32(rot)))))
        s = float(np.float32(np.sin(np.float64(np.float32(rot)))))
        sc = float(np.float32(scale))
        want = pts.clone()
        want[:, 0] = (c * x + s * y) * sc
        want[:, 1] = (c * y - s * x) * sc
        want[:, 2] = pts[:, 2] * sc
        bound = 8 * U * (pts[:, 0].abs() + pts[:, 1].abs()) * abs(sc)
        got = ops.points_view_(pts.clone(), view)
        assert torch.equal(got[:, 3:], pts[:, 3:])
        assert bool(((got[:, 0] - want[:, 0]).abs() <= bound).all()) and bool(((got[:, 1] - want[:, 1]).abs() <= bound).all())
        assert bool(((got[:, 2] - want[:, 2]).abs() <= 2 * U * want[:, 2].abs()).all())
        if rot != 0.0:
            assert not torch.equal(got[:, :2], pts[:, :2])
    with pytest.raises(Exception):
        ops.points_view_(torch.zeros(4, 3), view)


def _without_exact_ties(z):
    """The golden's labels with every prediction that has two exactly tied candidates moved to label -1: a rounded view does
    not keep an exact tie."""
    labels = z["labels"].copy()
    for b in range(labels.shape[0]):
        rows = np.arange(z["ref_off"][b], z["ref_off"][b + 1])
        for t in range(labels.shape[1]):
            for i in range(int(z["counts"][b, t])):
                same = rows[z["ref_labels"][rows] == labels[b, t, i]]
                d = np.sort(np.linalg.norm(z["ref_boxes"][same, :2].astype(np.float64)
                                           - z["boxes"][b, t, i, :2].astype(np.float64), axis=1))
                if np.any(np.diff(d) == 0):
                    labels[b, t, i] = -1
    assert 0 < (labels != z["labels"]).sum() < 20
    return labels


@pytest.mark.parametrize("view", VIEWS + [(True, True, 0.0, 2.0)], ids=["flip_x", "flip_y_rot_scale", "all", "exact"])
def test_match_under_a_view_equals_the_identity(dev, z, view):
    """Predictions pushed forward through ``view`` (float64, rounded to float32 once) and matched with ``view=`` give the
    ``match_ref`` of the originals under the identity.  ``exact``: flips and a power-of-two scale round-trip exactly, so the
    golden's exact ties stay in and the result is the reference's own."""
    boxes, scores, labels, counts, rb, rl, rs, ro = golden_inputs(z)
    exact = view == (True, True, 0.0, 2.0)
    if not exact:
        labels = _without_exact_ties(z)
    moved = boxes.copy()
    moved[..., :3] = PN.view_points(boxes[..., :3], view).astype(np.float32)
    moved[..., 3:6] = (boxes[..., 3:6].astype(np.float64) * view[3]).astype(np.float32)
    plain = run_kernel(dev, boxes, scores, labels, counts, rb, rl, rs, ro)
    got = run_kernel(dev, moved, scores, labels, counts, rb, rl, rs, ro, view=view)
    assert np.array_equal(got["match_ref"], plain["match_ref"]) and np.array_equal(got["cls_count"], plain["cls_count"])
    assert (plain["match_ref"] >= 0).sum() > 50
    hit = (plain["match_ref"] >= 0) & (plain["match_ref"] == z["match_ref"])
    assert np.all(np.abs(got["match_iou"][hit] - z["match_iou"][hit]) <= 64 * U * z["match_iou"][hit])
    if exact:
        assert np.array_equal(got["match_ref"], z["match_ref"])
    else:
        want = PN.match_frames(moved, scores, labels, counts, rb, rl, rs, ro, NCLS, view=view)
        check(got, want, "view")


# ------------------------------------------------------------------------------------------------ loaders and selector
@pytest.fixture(scope="module")
def cbgs(dev):
    from al3d import synthetic
    from al3d.datasets import PoolFrames, generate_task_anchors
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "cbgs_cald.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    model = model.to(dev).eval()
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])
    pool = PoolFrames.from_synthetic(16, dev, num_base=4, seed=3, nsweeps=1)
    return cfg, model, anchors, pool


def test_device_loader_view_none_is_todays_batches(dev, cbgs):
    """``view=None`` launches nothing: the batch is what the voxelizer gives for the pool's own points (today's path), bit
    for bit; a view changes the voxels and leaves the pool's points alone."""
    from al3d.datasets import DeviceSweepLoader
    cfg, _, anchors, pool = cbgs
    ids = [2, 3, 4, 5]
    flat = pool.flat.clone()
    keys = ("voxel_features", "coordinates", "num_points", "num_voxels")

    def grab(ld):                                        # copies: a voxelizer may hand out its own buffers again
        ex = next(iter(ld))
        return {k: ex[k].clone() for k in keys}

    default = grab(DeviceSweepLoader(pool, cfg.voxel_generator, anchors, 4, indices=ids, device=dev))
    loader = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, 4, indices=ids, device=dev, view=None)
    none = grab(loader)
    pts = pool.flat[pool.offsets[2]:pool.offsets[6]]
    off = torch.tensor([pool.offsets[i] - pool.offsets[2] for i in range(2, 7)], dtype=torch.int64, device=dev)
    v = loader.voxelizer(pts, off, want_voxels=False)
    for k, w in zip(keys, (v["feat"], v["coords"], v["num_points"], v["num_voxels"])):
        n = int(v["num_voxels"].sum()) if k != "num_voxels" else None
        for ex in (default, none):
            assert torch.equal(ex[k][:n], w[:n]), k
    loader.view = (True, False, 0.3, 0.95)
    moved = grab(loader)
    assert not torch.equal(moved["num_voxels"], none["num_voxels"]) or \
        not torch.equal(moved["coordinates"], none["coordinates"])
    assert torch.equal(pool.flat, flat)
    loader.view = (False, False, 0.0, 1.0)               # the identity view runs the kernel and changes no bit
    same = grab(loader)
    for k in keys:
        assert torch.equal(same[k], none[k]), k


def test_file_loader_view(dev, cbgs, tmp_path):
    """``FileSweepLoader(view=)`` on a small on-disk pool (ragged last batch): the merged points it yields are the plain
    loader's points through ``points_view_``, and its voxels are those of ``DeviceSweepLoader(view=)`` on the same clouds;
    ``view=None`` yields the plain loader's batches."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from write_synthetic_pool import write_pool
    from al3d import selector_ops as ops
    from al3d.datasets import DeviceSweepLoader, FileSweepLoader, PoolFrames
    cfg, _, anchors, _ = cbgs
    root = str(tmp_path / "pool")
    infos, _ = write_pool(root, scenes=1, base=2, nsweeps=2)
    infos = infos[:3]
    view = (True, False, 0.3, 0.95)
    keys = ("voxel_features", "coordinates", "num_points", "num_voxels")

    def run(ld):
        out = []
        for ex in ld:
            off = ex["point_offsets"].cpu().numpy()
            out.append(({k: ex[k].clone() for k in keys}, ex["points"][:off[-1]].clone(), off))
        return out

    kw = dict(batch_size=2, device=dev, root=root, threads=2, depth=2, nsweeps=2)
    plain = run(FileSweepLoader(infos, cfg.voxel_generator, anchors, **kw))
    none = run(FileSweepLoader(infos, cfg.voxel_generator, anchors, view=None, **kw))
    moved = run(FileSweepLoader(infos, cfg.voxel_generator, anchors, view=view, **kw))
    assert len(plain) == len(moved) == 2
    clouds = [p[1][o[b]:o[b + 1]].cpu().numpy() for p in plain for o in [p[2]] for b in range(len(o) - 1)]
    ref = list(DeviceSweepLoader(PoolFrames.from_numpy(clouds, dev), cfg.voxel_generator, anchors, 2, device=dev, view=view))
    for a, n, m, r in zip(plain, none, moved, ref):
        assert torch.equal(m[1], ops.points_view_(a[1].clone(), view)) and not torch.equal(m[1], a[1])
        for k in keys:
            assert torch.equal(a[0][k], n[0][k]) and torch.equal(m[0][k], r[k]), k


def test_ppal_prepass_end_to_end(dev, cbgs, tmp_path):
    """``run_ppal_prepass`` on the 16-frame pool with the sweep's own detections written into the infos as ground truth
    (``gt_boxes`` / ``gt_names``): every detection is its own nearest reference at distance 0 with scale IoU 1, so a match's
    quality is ``score^0.6`` and the weights follow from the labelled frames' scores alone (float64 here).  Tolerance: the
    kernel's per-class sum is within (n + 16) 2^-23 <= 1.2e-5 relative (n <= 83 boxes per task), the mean quality q
    likewise, and |dw/dq| = 6 b / (b (1 - q) + 1) <= 6 b = 2.4, so the weights agree to 3e-5; 1e-4 is asserted.  The file
    reads back the way ``PPALSelector.buffer_pred`` reads it."""
    from al3d import synthetic
    from al3d.datasets import DeviceSweepLoader
    from al3d.selectors import prepass as P
    cfg, model, anchors, pool = cbgs
    loader = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, 8, device=dev)
    names = P.head_class_names(model)
    assert names == list(cfg.class_names) and len(names) == NCLS
    dets = P.sweep_detections(model, loader, dev, 16)
    infos = synthetic.make_pool(1, seed=4)[0][:16]
    for i, info in enumerate(infos):
        rows = slice(dets.off[i], dets.off[i + 1])
        info["gt_boxes"] = dets.boxes[rows]
        info["gt_names"] = np.array([names[c] for c in dets.labels[rows]], dtype="<U32")
    labelled = [3, 5]
    path = str(tmp_path / "w" / "diff_category_average.json")
    got = P.run_ppal_prepass(model, loader, dev, infos, labelled, path)
    want = {}
    b = np.exp(1.0 / 3.0) - 1
    for c, name in enumerate(names):
        s = np.concatenate([dets.scores[dets.off[i]:dets.off[i + 1]][dets.labels[dets.off[i]:dets.off[i + 1]] == c]
                            for i in labelled]).astype(np.float64)
        if len(s):
            want[name] = 1 + 3.0 * np.log(b * (1.0 - np.mean(s ** 0.6)) + 1) * 2.0
    assert set(got) == set(want) and len(want) >= 3
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-4, (k, got[k], want[k])
    with open(path, "r") as f:
        class_weight = json.load(f)
    assert [class_weight[c] for c in got] == list(got.values())


def test_cald_selector_prepass_end_to_end(dev, cbgs, tmp_path):
    """``CaldSelector(prepass=True)`` on a 16-frame synthetic pool (one batch shape) writes both files and selects what a
    second ``CaldSelector`` selects replaying them.  The view is the identity, passed as a view: both sweeps then see the
    same voxels, every detection matches itself, and every frame with a detection enters the divergence ranking."""
    from al3d import synthetic
    from al3d.datasets import DeviceSweepLoader
    from al3d.selectors import build_selector
    cfg, model, anchors, pool = cbgs
    infos = synthetic.make_pool(1, seed=4)[0][:16]
    ip, bp = str(tmp_path / "infos.pkl"), str(tmp_path / "buffer.json")
    pickle.dump(infos, open(ip, "wb"))
    json.dump({"0": [], "2": [3]}, open(bp, "w"))
    sp, jp = str(tmp_path / "files" / "sorted.json"), str(tmp_path / "files" / "jsdiv.pkl")
    loader = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, 8, device=dev)
    common = dict(type="CaldSelector", budget=E2E_BUDGET, buffer_file=bp, infos_origin=ip, buffer_path=sp, jsdiv_path=jp)
    sel = build_selector(dict(common, detector=model, dataloader=loader, prepass=True,
                              prepass_view=(False, False, 0.0, 1.0)))
    sel.select_samples(local_rank=0)
    ranking = json.load(open(sp))
    jsdiv = pickle.load(open(jp, "rb"))
    assert sorted(ranking) == list(range(16)) and set(jsdiv) <= set(range(16)) and len(jsdiv) >= 8
    assert all(np.isfinite(v) and v >= 0 for v in jsdiv.values())
    assert loader.view is None and sel.detector is None
    picked = sel.selected_index[sel.current_budget]
    assert picked[-1] == 3 and len(picked) >= 3 and len(set(picked)) == len(picked)
    replay = build_selector(dict(common))
    replay.select_samples(local_rank=0)
    assert replay.selected_index[replay.current_budget] == picked
    # the identity view: a detection is its own nearest reference at distance 0 and scale IoU 1, so a frame's consistency
    # is min |1 + s - 1.3| over its detections and the ranking is ascending in it
    from al3d.selectors.prepass import sweep_detections, sweep_matches
    refs = sweep_detections(model, loader, dev, 16)
    m = sweep_matches(model, loader, dev, refs, view=(False, False, 0.0, 1.0))
    assert m["cls_count"].shape == (16, NCLS) and np.array_equal(m["cls_count"].sum(1), np.diff(refs.off))
    cons = np.minimum(1.0, m["cls_cons"].min(1).astype(np.float64))
    want = np.array([np.abs(1.0 + refs.scores[refs.off[i]:refs.off[i + 1]].astype(np.float64) - 1.3).min()
                     if refs.off[i + 1] > refs.off[i] else 1.0 for i in range(16)])
    assert np.all(np.abs(cons - np.minimum(1.0, want)) <= 5e-6)
    assert ranking == [int(i) for i in np.argsort(cons, kind="stable")]

