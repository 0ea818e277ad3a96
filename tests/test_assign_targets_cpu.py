"""CPU suite of anchor target assignment: the numpy restatement and the host mirrors (al3d.ops.box_np_ops, the box coder, the
anchor generator) against the reference's golden, the refusals, the argument checks of the C entry (they run before any
launch), and AssignTarget's two modes up to the device call."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_targets_numpy as Y  # noqa: E402

CASES = Y.load_golden()
IDS = [c["name"] for c in CASES]


def make_coder(case):
    from al3d.models.box_coder import GroundBox3dCoderTorch
    c = case["coder"]
    return GroundBox3dCoderTorch(linear_dim=c["linear"], vec_encode=c["vec"], n_dim=c["n_dim"], norm_velo=c["norm_velo"])


def make_generators(case, task):
    from al3d.datasets.anchors import AnchorGeneratorRange
    r = case["meta"]["range"]
    return [AnchorGeneratorRange(anchor_ranges=[r[0], r[1], c["z"], r[2], r[3], c["z"]], sizes=c["sizes"],
                                 rotations=c["rotations"], velocities=[0, 0] if case["coder"]["n_dim"] == 9 else None,
                                 class_name=c["class_name"], match_threshold=float(c["matched"]),
                                 unmatch_threshold=float(c["unmatched"])) for c in task]


def test_golden_holds_the_cases_the_issue_lists():
    assert IDS == ["edge7", "thr9", "lin16", "one7"]
    by = {c["name"]: c for c in CASES}
    assert by["edge7"]["tasks"][0][0]["anchors"].shape == (1, 5, 7, 2, 7)            # 70 anchors per class
    assert by["lin16"]["tasks"][0][0]["anchors"].shape == (1, 16, 16, 2, 9)          # 512
    assert by["thr9"]["meta"]["B"] == 3 and [len(f[0]) for f in by["thr9"]["frames"]] == [7, 0, 3]
    assert [len(t) for t in by["thr9"]["tasks"]] == [2, 1]
    assert np.isnan(by["thr9"]["frames"][0][0]).sum() == 1
    assert os.path.getsize(Y.GOLDEN) < 1 << 20


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_the_reference(case):
    got = Y.assign_batch(case["tasks"], case["coder"], case["frames"])
    Y.compare_to_golden(case, got)
    # numpy's own float32 library on both sides: every column is the reference's, bit for bit
    for t in range(len(case["tasks"])):
        assert np.array_equal(got["reg_targets"][t].view(np.int32), case["reg_targets"][t].view(np.int32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_box_np_ops_and_coder_mirrors_equal_the_reference(case):
    """near boxes + iou_jit(eps=0) reproduce every encoded anchor's box (first maximum), and the coder's ``encode`` its code."""
    from al3d.ops import box_np_ops as B
    coder = make_coder(case)
    nd = case["coder"]["n_dim"]
    for t, classes in enumerate(case["tasks"]):
        stride = sum(c["anchors"].shape[-2] for c in classes)
        slot = 0
        for c in classes:
            a = c["anchors"].reshape(-1, nd)
            num_rot = c["anchors"].shape[-2]
            for b, (boxes, names) in enumerate(case["frames"]):
                rows = np.where(names == c["class_name"])[0]
                if len(rows) == 0:
                    continue
                g = boxes[rows].copy()
                g[:, -1] = B.limit_period(g[:, -1], offset=0.5, period=np.pi * 2)
                g = np.nan_to_num(g)
                ov = B.iou_jit(B.rbbox2d_to_near_bbox(a[:, [0, 1, 3, 4, -1]]), B.rbbox2d_to_near_bbox(g[:, [0, 1, 3, 4, -1]]), eps=0.0)
                assert ov.dtype == np.float32
                assert np.array_equal(ov, Y.iou(Y.near_bbox(a[:, [0, 1, 3, 4, -1]]), Y.near_bbox(g[:, [0, 1, 3, 4, -1]])))
                sel = lambda v: v[b].reshape(-1, stride, *v.shape[2:])[:, slot:slot + num_rot].reshape(-1, *v.shape[2:])  # noqa: E731
                gi, want = sel(case["gt_index"][t]), sel(case["reg_targets"][t])
                fg = np.where(gi >= 0)[0]
                assert np.array_equal(rows[ov.argmax(axis=1)[fg]], gi[fg])
                code = coder.encode(g[ov.argmax(axis=1)[fg]], a[fg])
                assert code.dtype == np.float32 and np.array_equal(code.view(np.int32), want[fg].view(np.int32))
            slot += num_rot


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_encode_torch_and_generated_anchors(case):
    import torch
    from al3d.datasets.target_assigner import NearestIouSimilarity, TargetAssigner
    coder = make_coder(case)
    for task in case["tasks"]:
        ta = TargetAssigner(box_coder=coder, anchor_generators=make_generators(case, task),
                            region_similarity_calculator=NearestIouSimilarity(), device="cpu")
        assert ta.classes == [c["class_name"] for c in task]
        d = ta.generate_anchors_dict([1, *case["meta"]["fm"]])
        for c in task:
            got = d[c["class_name"]]
            assert np.array_equal(got["anchors"].view(np.int32), c["anchors"].view(np.int32))
            assert got["matched_thresholds"].dtype == np.float32 and got["matched_thresholds"][0] == c["matched"]
            assert got["unmatched_thresholds"][0] == c["unmatched"]
        whole = ta.generate_anchors([1, *case["meta"]["fm"]])
        assert whole["anchors"].shape[-2] == ta.num_anchors_per_location
    if not case["coder"]["norm_velo"]:
        a = case["tasks"][0][0]["anchors"].reshape(-1, case["coder"]["n_dim"])[:8]
        g = a + np.float32(0.25)
        want = coder.encode(g, a)
        got = coder.encode_torch(torch.from_numpy(g), torch.from_numpy(a)).numpy()
        assert np.allclose(got, want, rtol=0, atol=1e-6)


def test_refusals_name_the_option():
    from al3d.datasets.target_assigner import NearestIouSimilarity, TargetAssigner, build_similarity_metric
    case = CASES[0]
    coder, gens = make_coder(case), make_generators(case, case["tasks"][0])
    with pytest.raises(NotImplementedError, match="positive_fraction"):
        TargetAssigner(coder, gens, NearestIouSimilarity(), positive_fraction=0.5)
    with pytest.raises(NotImplementedError, match="region_similarity_calculator"):
        TargetAssigner(coder, gens, region_similarity_calculator=object())
    with pytest.raises(NotImplementedError, match="rotate_iou_similarity"):
        build_similarity_metric(dict(type="rotate_iou_similarity"))
    ta = TargetAssigner(coder, gens, device="cpu")                    # the default (None) is the one similarity that is built
    assert isinstance(ta._region_similarity_calculator, NearestIouSimilarity)
    d = ta.generate_anchors_dict([1, 5, 7])
    with pytest.raises(ValueError, match="gt_names"):
        ta.assign_v2(d, np.zeros((0, 7), np.float32))
    with pytest.raises(ValueError, match="gt_names"):
        ta.assign_v2(d, np.zeros((2, 7), np.float32), gt_names=["car"])
    from al3d import lib
    from al3d.detector_ops import AssignPlan
    with pytest.raises(lib.Al3dError, match="twice"):
        AssignPlan([ta.plan_classes(d), ta.plan_classes(d)], coder, "cpu")
    with pytest.raises(NotImplementedError, match="anchors_mask"):
        ta.assign_v2(d, np.zeros((0, 7), np.float32), anchors_mask=np.ones(70, bool), gt_classes=np.zeros(0, np.int32), gt_names=[])


def test_entry_refuses_bad_arguments_before_any_launch():
    Y_bad = Y.bad_argument_calls()
    from al3d import lib
    so = lib.load()
    assert len(Y_bad) >= 8
    for what, args, word in Y_bad:
        assert so.al3d_assign_targets_f32(*args) == -1, what
        assert word in so.al3d_last_error(), (what, so.al3d_last_error())
    for what, args in Y.bad_launch_calls():
        assert so.al3d_assign_targets_launch_f32(*args) == -1, what
        assert b"groups" in so.al3d_last_error()


def _assigner_cfg(case):
    r = case["meta"]["range"]
    nd = case["coder"]["n_dim"]
    gens = [dict(type="anchor_generator_range", sizes=c["sizes"], anchor_ranges=[r[0], r[1], c["z"], r[2], r[3], c["z"]],
                 rotations=c["rotations"], matched_threshold=float(c["matched"]), unmatched_threshold=float(c["unmatched"]),
                 class_name=c["class_name"], **(dict(velocities=[0, 0]) if nd == 9 else {}))
            for t in case["tasks"] for c in t]
    tasks = [dict(num_class=len(t), class_names=[c["class_name"] for c in t]) for t in case["tasks"]]
    co = case["coder"]
    return dict(box_coder=dict(type="ground_box3d_coder", n_dim=nd, linear_dim=co["linear"], encode_angle_vector=co["vec"],
                               norm_velo=co["norm_velo"]),
                target_assigner=dict(type="iou", anchor_generators=gens, sample_positive_fraction=-1, sample_size=512,
                                     region_similarity_calculator=dict(type="nearest_iou_similarity"), pos_area_threshold=-1,
                                     tasks=tasks),
                out_size_factor=8, debug=False)


def test_assign_target_val_mode_is_anchors_only():
    import torch
    from al3d.datasets import AssignTarget, Reformat, generate_task_anchors
    case = [c for c in CASES if c["name"] == "thr9"][0]
    cfg = _assigner_cfg(case)
    stage = AssignTarget(cfg=cfg, device="cpu")
    for mode in ({}, {"mode": "val"}):
        res = dict(lidar=dict(voxels=dict(shape=np.array([56, 40, 8]), voxels=None, num_points=None, num_voxels=None,
                                          coordinates=None), annotations=None), **mode)
        out, _ = stage(res, {})
        assert set(out["lidar"]["targets"]) == {"anchors"}
        want = generate_task_anchors(cfg["target_assigner"]["tasks"], cfg["target_assigner"]["anchor_generators"], [1, 5, 7])
        assert len(out["lidar"]["targets"]["anchors"]) == 2
        for a, w in zip(out["lidar"]["targets"]["anchors"], want):
            assert a.dtype == torch.float32 and np.array_equal(a.numpy(), w)
        ex, _ = Reformat()(out, {})
        assert "labels" not in ex and ex["anchors"] is out["lidar"]["targets"]["anchors"]
    assert stage._plans == {}                            # val mode never builds the train side
    # train mode without the three annotation arrays: anchors only, like val
    for ann in (None, {}, dict(gt_boxes=np.zeros((0, 9), np.float32))):
        res = dict(mode="train", lidar=dict(voxels=dict(shape=np.array([56, 40, 8])), annotations=ann))
        out, _ = stage(res, {})
        assert set(out["lidar"]["targets"]) == {"anchors"} and stage._plans == {}


def test_assign_target_train_mode_splits_by_task_and_calls_the_device(monkeypatch):
    """preprocess.py:380-424 on hand-set annotations; the device call is recorded, not run (no GPU here)."""
    import torch
    from al3d import detector_ops
    from al3d.datasets import AssignTarget, Reformat
    case = [c for c in CASES if c["name"] == "thr9"][0]
    stage = AssignTarget(cfg=_assigner_cfg(case), device="cpu")
    boxes, names = case["frames"][0]
    order = ["e1", "e2", "ped"]
    classes = np.array([order.index(n) + 1 for n in names], dtype=np.int32)
    seen = {}

    def fake(plan, gt_boxes, gt_names=None, gt_class=None, limit_angle=True, launch=None, with_index=True):
        seen.update(plan=plan, boxes=gt_boxes, cls=gt_class, limit=limit_angle)
        return dict(labels=[torch.zeros(1, n, dtype=torch.int32) for n in plan.task_anchors],
                    reg_targets=[torch.zeros(1, n, plan.code_size) for n in plan.task_anchors],
                    reg_weights=[torch.zeros(1, n) for n in plan.task_anchors])

    monkeypatch.setattr(detector_ops, "assign_targets", fake)
    res = dict(mode="train", lidar=dict(voxels=dict(shape=np.array([56, 40, 8]), voxels=None, num_points=None, num_voxels=None,
                                                    coordinates=None),
                                        annotations=dict(gt_boxes=boxes.copy(), gt_classes=classes, gt_names=names.copy())))
    out, _ = stage(res, {})
    ann = out["lidar"]["annotations"]
    assert [list(n) for n in ann["gt_names"]] == [["e1", "e1", "e2", "e2", "e2"], ["ped", "ped"]]
    assert [list(c) for c in ann["gt_classes"]] == [[1, 1, 2, 2, 2], [1, 1]]
    assert np.array_equal(ann["gt_boxes"][1][:, -1], Y.limit_period(boxes[[4, 5], -1], 0.5, np.pi * 2))
    assert seen["limit"] is False and list(seen["cls"][0]) == [0, 0, 1, 1, 1, 2, 2]
    assert seen["plan"].task_anchors == [5 * 7 * 4, 5 * 7 * 1] and seen["plan"].class_names == order
    assert [r["slot_offset"] for r in seen["plan"].rows] == [0, 2, 0] and [r["label"] for r in seen["plan"].rows] == [1, 2, 1]
    t = out["lidar"]["targets"]
    assert set(t) == {"anchors", "labels", "reg_targets", "reg_weights"} and t["reg_targets"][0].shape == (140, 10)
    ex, _ = Reformat()(out, {})
    assert ex["labels"] is t["labels"] and ex["reg_weights"] is t["reg_weights"]


def test_preprocess_train_still_refuses():
    from al3d.datasets import Compose
    with pytest.raises(NotImplementedError):
        Compose([dict(type="Preprocess", cfg=dict(mode="train"))])


def test_struct_layout_matches_the_header():
    from al3d.detector_ops import AssignClass
    assert ctypes.sizeof(AssignClass) == 48 and AssignClass.anchor_begin.offset == 8 and AssignClass.unmatched.offset == 40
