"""GPU suite of anchor target assignment (csrc/assign_targets.hip behind detector_ops.assign_targets, TargetAssigner.assign_v2,
AssignTarget's train mode, FileSweepLoader(with_targets=True)).

labels, reg_weights, gt_index and the code columns made of + - * / sqrt are compared bit for bit with the reference's golden
(tests/golden/assign_targets.npz); the log / cos / sin columns within the golden's own float32 error plus 4 float32 ulps of
the float64 yardstick (assign_targets_numpy.allowed_error).  At sizes the golden does not have the kernel owes the numpy
restatement, which tests/test_assign_targets_cpu.py pins to the same golden."""
import os
import sys

import numpy as np
import pytest
import torch

import assign_targets_numpy as Y
from test_assign_targets_cpu import _assigner_cfg, make_coder, make_generators

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = Y.load_golden()
IDS = [c["name"] for c in CASES]
KEYS = ("labels", "reg_targets", "reg_weights", "gt_index")


def _plan(tasks, coder):
    from al3d.detector_ops import AssignPlan
    return AssignPlan(tasks, coder, DEV)


def _run(plan, frames, launch=None, **kw):
    from al3d.detector_ops import assign_targets
    out = assign_targets(plan, [np.ascontiguousarray(f[0], dtype=np.float32).reshape(-1, plan.n_dim) for f in frames],
                         gt_names=[f[1] for f in frames], launch=launch, **kw)
    got = {k: [v.cpu().numpy() for v in out[k]] for k in KEYS}
    got["gt_overlap"] = out["gt_overlap"].cpu().numpy()
    return got


def _same_bytes(a, b, what):
    for k in KEYS:
        for t, (x, y) in enumerate(zip(a[k], b[k])):
            assert x.tobytes() == y.tobytes(), f"{what}: {k} of task {t} differs"
    assert a["gt_overlap"].tobytes() == b["gt_overlap"].tobytes(), f"{what}: gt_overlap differs"


def _compare_to_restatement(got, want, coder, frames, task_anchors, what):
    """Integer outputs, gt_overlap and the + - * / sqrt columns bit for bit.  The log / cos / sin columns against the same
    formula in float64 on the float32 inputs: numpy's own float32 error there plus 4 float32 ulps at the column's largest
    intermediate magnitude (1.0 for cos / sin, the largest |log| of the frame for the size columns).
    ``task_anchors``: per task the anchors in the task's output order."""
    exact, loose = Y.exact_columns(coder["n_dim"], coder["vec"], coder["linear"])
    for t in range(len(want["labels"])):
        for k in ("labels", "reg_weights", "gt_index"):
            assert got[k][t].tobytes() == want[k][t].tobytes(), f"{what}: {k} of task {t}"
        g, w = got["reg_targets"][t], want["reg_targets"][t]
        assert g.shape == w.shape
        for c in exact:
            assert np.array_equal(g[..., c].view(np.int32), w[..., c].view(np.int32)), f"{what}: exact column {c} of task {t}"
        for b, (boxes, _) in enumerate(frames):
            idx = want["gt_index"][t][b]
            fg = idx >= 0
            for c in loose:
                assert np.all(g[b][~fg][:, c] == 0)
            if not loose or not fg.any():
                continue
            boxes = np.array(boxes, np.float32)
            boxes[:, -1] = Y.limit_period(boxes[:, -1], 0.5, np.pi * 2)
            y64 = Y.encode(np.nan_to_num(boxes)[idx[fg]], task_anchors[t][fg], coder["vec"], coder["linear"], coder["norm_velo"],
                           np.float64)
            for c in loose:
                mag = 1.0 if c >= g.shape[-1] - 2 and coder["vec"] else max(float(np.abs(y64[:, 3:6]).max()), 2.0 ** -126)
                ulp = 2.0 ** np.floor(np.log2(mag)) * Y.F32_EPS
                own = float(np.abs(w[b][fg][:, c] - y64[:, c]).max())
                err = float(np.abs(g[b][fg][:, c] - y64[:, c]).max())
                print(f"{what}: task {t} frame {b} column {c}: error {err:.3e}, allowed {own + 4 * ulp:.3e} (numpy's own {own:.3e})")
                assert err <= own + 4 * ulp, f"{what}: task {t} frame {b} column {c}"
    gt = np.concatenate(want["gt_overlap"]) if len(want["gt_overlap"]) else np.zeros(0, np.float32)
    assert got["gt_overlap"].tobytes() == gt.astype(np.float32).tobytes(), f"{what}: gt_overlap"


def _task_order(plan):
    """Per task the plan's class-grouped anchors in the task's (location, class, rotation) output order."""
    out = [[] for _ in plan.task_anchors]
    for r, t in zip(plan.rows, plan.task_of):
        a = plan.anchors_np[r["anchor_begin"]:r["anchor_begin"] + r["num_loc"] * r["num_rot"]]
        out[t].append(a.reshape(r["num_loc"], r["num_rot"], -1))
    return [np.concatenate(v, axis=1).reshape(-1, v[0].shape[-1]) for v in out]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_entry_equals_the_reference(case):
    """The C entry, default launch shape, on every golden case (the whole batch in one call)."""
    got = _run(_plan(case["tasks"], make_coder(case)), case["frames"])
    Y.compare_to_golden(case, got)
    want = Y.assign_batch(case["tasks"], case["coder"], case["frames"])
    assert got["gt_overlap"].tobytes() == np.concatenate(want["gt_overlap"]).tobytes()


@pytest.mark.parametrize("case", [c for c in CASES if c["name"] in ("thr9", "one7")], ids=["thr9", "one7"])
def test_launch_shapes_and_runs_give_the_same_bytes(case):
    """groups / threads / chunk change nothing, nor does a second run.  chunk 1 is the smallest the entry accepts: one7's
    two boxes of one class are one more than it, thr9 has up to three of a class."""
    plan = _plan(case["tasks"], make_coder(case))
    base = _run(plan, case["frames"])
    Y.compare_to_golden(case, base)
    _same_bytes(base, _run(plan, case["frames"]), "second run")
    for launch in ((1, 64, 1), (3, 192, 2), (7, 1024, 256), (4096, 256, 1)):
        _same_bytes(base, _run(plan, case["frames"], launch=launch), f"launch {launch}")
    no_index = _run(plan, case["frames"], with_index=False)
    assert no_index["gt_index"] == [] and no_index["labels"][0].tobytes() == base["labels"][0].tobytes()


def test_chunks_are_crossed_inside_a_64_row_step_and_at_its_end():
    """70 + 64 boxes of two classes interleaved with boxes of no class (5 x 7 map): a class's list crosses the chunk in the
    middle of a 64-row step (chunk 5, 64) and exactly at the end of one (chunk 32), and fits (256)."""
    case = [c for c in CASES if c["name"] == "one7"][0]
    rng = np.random.default_rng(3)
    boxes, names = [], []
    for i in range(70 + 64 + 30):
        name = ("van", "bike", "none")[0 if i % 7 in (0, 2, 4) else 1 if i % 7 in (1, 3, 5) else 2]
        if names.count(name) >= {"van": 70, "bike": 64, "none": 30}[name]:
            name = "van" if names.count("van") < 70 else "bike" if names.count("bike") < 64 else "none"
        size = [2.0, 4.5] if name == "van" else [0.6, 1.8]
        boxes.append([*rng.uniform(0, 28, 1), *rng.uniform(0, 20, 1), -1.0, *(rng.uniform(0.8, 1.25, 2) * size), 1.5,
                      rng.uniform(-4, 4)])
        names.append(name)
    boxes[10] = boxes[3]                                           # a duplicate: ties go to the first copy
    frames = [(np.array(boxes, np.float32), np.array(names)), (np.zeros((0, 7), np.float32), np.array([], dtype="<U4")),
              (np.array(boxes[:5], np.float32), np.array(names[:5]))]
    assert names.count("van") == 70 and names.count("bike") == 64
    plan = _plan(case["tasks"], make_coder(case))
    want = Y.assign_batch(case["tasks"], case["coder"], frames)
    base = _run(plan, frames)
    _compare_to_restatement(base, want, case["coder"], frames, _task_order(plan), "default")
    assert np.array_equal(base["reg_targets"][0].view(np.int32), want["reg_targets"][0].view(np.int32))   # linear + scalar: all exact
    for launch in ((2, 128, 5), (6, 256, 64), (1, 512, 32), (5, 64, 69)):
        _same_bytes(base, _run(plan, frames, launch=launch), f"launch {launch}")


def test_more_frames_than_one_launch_carries():
    """B = 257 on the 5 x 7 map: the entry splits the batch into launches of 256 frames, whose offsets travel in the kernel
    arguments.  Boxes sit in frames 0, 255 and 256 (the last frame of the first launch, the only frame of the second), the
    rest are empty; every frame's rows must equal the restatement's, and the first 256 those of a B = 256 call."""
    case = [c for c in CASES if c["name"] == "one7"][0]
    full = case["frames"][0]
    empty = (np.zeros((0, 7), np.float32), np.array([], dtype="<U4"))
    frames = [empty] * 257
    frames[0] = full
    frames[255] = (full[0][1:], full[1][1:])
    frames[256] = (full[0][[2, 0]], full[1][[2, 0]])
    plan = _plan(case["tasks"], make_coder(case))
    got = _run(plan, frames)
    want = Y.assign_batch(case["tasks"], case["coder"], frames)
    _compare_to_restatement(got, want, case["coder"], frames, _task_order(plan), "B = 257")
    assert got["labels"][0].shape == (257, 140) and (got["labels"][0][256] > 0).any() and (got["labels"][0][255] > 0).any()
    assert np.all(got["labels"][0][1:255] == 0) and np.all(got["gt_index"][0][1:255] == -1)
    one = _run(plan, frames[:256])
    for k in KEYS:
        assert got[k][0][:256].tobytes() == one[k][0].tobytes(), k
    _same_bytes(got, _run(plan, frames, launch=(5, 128, 1)), "launch (5, 128, 1)")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_assign_v2_and_assign_target_train_equal_the_reference(case):
    """Frame by frame: TargetAssigner.assign_v2 per task on the regrouped, angle-limited boxes (as AssignTarget hands them
    over), and AssignTarget's train mode from the frame's annotations, against the golden's dicts."""
    from al3d.datasets import AssignTarget, Reformat
    from al3d.datasets.target_assigner import NearestIouSimilarity, TargetAssigner
    coder = make_coder(case)
    fm = [1, *case["meta"]["fm"]]
    order = [c["class_name"] for t in case["tasks"] for c in t]
    stage = AssignTarget(cfg=_assigner_cfg(case), device=DEV)
    for b, (boxes, names) in enumerate(case["frames"]):
        known = np.array([n in order for n in names], dtype=bool)
        boxes, names = boxes[known], names[known]
        one = dict(case, labels=[v[b:b + 1] for v in case["labels"]], reg_targets=[v[b:b + 1] for v in case["reg_targets"]],
                   reg_weights=[v[b:b + 1] for v in case["reg_weights"]], targets64=[v[b:b + 1] for v in case["targets64"]])
        got = dict(labels=[], reg_targets=[], reg_weights=[])
        for task in case["tasks"]:
            ta = TargetAssigner(box_coder=coder, anchor_generators=make_generators(case, task),
                                region_similarity_calculator=NearestIouSimilarity(), device=DEV)
            tn = [c["class_name"] for c in task]
            rows = np.concatenate([np.where(names == n)[0] for n in tn]).astype(np.int64)
            tb = boxes[rows].copy()
            tb[:, -1] = Y.limit_period(tb[:, -1], offset=0.5, period=np.pi * 2)
            r = ta.assign_v2(ta.generate_anchors_dict(fm), tb, None, gt_classes=np.array([tn.index(n) + 1 for n in names[rows]]),
                             gt_names=names[rows])
            assert set(r) == {"labels", "bbox_targets", "bbox_outside_weights"} and r["labels"].dtype == np.int32
            got["labels"].append(r["labels"][None])
            got["reg_targets"].append(r["bbox_targets"][None])
            got["reg_weights"].append(r["bbox_outside_weights"][None])
        Y.compare_to_golden(one, got, where=f"assign_v2 frame {b}: ")
        res = dict(mode="train", lidar=dict(
            voxels=dict(shape=np.array([case["meta"]["fm"][1] * 8, case["meta"]["fm"][0] * 8, 8]), voxels=None, num_points=None,
                        num_voxels=None, coordinates=None),
            annotations=dict(gt_boxes=boxes.copy(), gt_classes=np.array([order.index(n) + 1 for n in names], dtype=np.int32),
                             gt_names=names.copy())))
        ex, _ = Reformat()(*stage(res, {}))
        assert isinstance(ex["labels"], list) and ex["labels"][0].is_cuda and ex["labels"][0].dim() == 1
        Y.compare_to_golden(one, {k: [v.cpu().numpy()[None] for v in ex[k]] for k in ("labels", "reg_targets", "reg_weights")},
                            where=f"AssignTarget frame {b}: ")


def _cbgs():
    from al3d.utils import Config
    return Config.fromfile(os.path.join(ROOT, "examples", "active", "cbgs_spatial_temporal_feature.py"))


def _scene_boxes(rng, n, names, sizes):
    out_b, out_n = [], []
    for _ in range(n):
        k = int(rng.integers(len(names)))
        w, l, h = np.array(sizes[k]) * rng.uniform(0.85, 1.2, 3)
        out_b.append([*rng.uniform(-45, 45, 2), rng.uniform(-2, 0), w, l, h, *rng.normal(0, 2, 2), rng.uniform(-7, 7)])
        out_n.append(names[k])
    return np.array(out_b, np.float32).reshape(-1, 9), np.array(out_n, dtype="<U32")


def _restatement_tasks(cfg):
    """The CBGS config's tasks for assign_targets_numpy.assign_batch, anchors from the package's generator."""
    from al3d.datasets.anchors import build_anchor_generator
    gens = {g["class_name"]: g for g in cfg.target_assigner.anchor_generators}
    tasks = []
    for t in cfg.tasks:
        classes = []
        for n in t["class_names"]:
            a = build_anchor_generator(gens[n]).generate([1, 128, 128])
            classes.append(dict(class_name=n, anchors=a.reshape([*a.shape[:3], -1, a.shape[-1]]),
                                matched=gens[n]["matched_threshold"], unmatched=gens[n]["unmatched_threshold"]))
        tasks.append(classes)
    return tasks


def test_full_size_two_class_task_equals_the_restatement():
    """128 x 128 map, one task of two classes (the config's truck / construction_vehicle), one frame of 40 boxes."""
    cfg = _cbgs()
    tasks = [_restatement_tasks(cfg)[1]]
    coder = dict(n_dim=9, vec=True, linear=False, norm_velo=False)
    names = [c["class_name"] for c in tasks[0]]
    sizes = [[2.51, 6.93, 2.84], [2.85, 6.37, 3.19]]
    frames = [_scene_boxes(np.random.default_rng(40), 40, names, sizes)]
    from al3d.models.box_coder import GroundBox3dCoderTorch
    plan = _plan(tasks, GroundBox3dCoderTorch(False, True, n_dim=9))
    got = _run(plan, frames)
    want = Y.assign_batch(tasks, coder, frames)
    assert got["labels"][0].shape == (1, 128 * 128 * 4)
    assert (want["labels"][0] > 0).sum() >= 40 and (want["labels"][0] == -1).sum() > 0
    _compare_to_restatement(got, want, coder, frames, _task_order(plan), "full size")


def test_loader_with_targets_equals_the_restatement(tmp_path):
    """FileSweepLoader(with_targets=True) on a 3-frame on-disk pool (batch 2 + 1) with the CBGS config: 6 tasks / 10
    classes at 128 x 128; a frame without boxes, a name no task carries, a NaN velocity."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from write_synthetic_pool import write_pool
    from al3d.datasets import FileSweepLoader, generate_task_anchors
    cfg = _cbgs()
    root = str(tmp_path / "pool")
    infos, _ = write_pool(root, scenes=1, base=2, nsweeps=2)
    infos = infos[:3]
    gens = cfg.target_assigner.anchor_generators
    names, sizes = [g["class_name"] for g in gens], [g["sizes"] for g in gens]
    rng = np.random.default_rng(8)
    for i, n in zip(range(3), (12, 0, 7)):
        infos[i]["gt_boxes"], infos[i]["gt_names"] = _scene_boxes(rng, n, names + ["animal"], sizes + [[0.5, 1.0, 0.5]])
    infos[0]["gt_boxes"][2, 6] = np.nan
    anchors = generate_task_anchors(cfg.tasks, gens, [1, 128, 128])
    kw = dict(batch_size=2, device=DEV, root=root, threads=2, depth=2, nsweeps=2)
    plain = list(FileSweepLoader(infos, cfg.voxel_generator, anchors, **kw))
    assert all("labels" not in ex and "gt_index" not in ex for ex in plain)          # default off: examples unchanged
    with pytest.raises(ValueError, match="target_cfg"):
        FileSweepLoader(infos, cfg.voxel_generator, anchors, with_targets=True, **kw)
    batches = list(FileSweepLoader(infos, cfg.voxel_generator, anchors, with_targets=True, target_cfg=cfg.assigner, **kw))
    assert [len(ex["metadata"]) for ex in batches] == [2, 1]
    tasks = _restatement_tasks(cfg)
    coder = dict(n_dim=9, vec=True, linear=False, norm_velo=False)
    for ex, p, ids in zip(batches, plain, ((0, 1), (2,))):
        assert set(ex) - set(p) == {"labels", "reg_targets", "reg_weights", "gt_index"}
        assert torch.equal(ex["voxel_features"], p["voxel_features"]) and torch.equal(ex["coordinates"], p["coordinates"])
        frames = [(infos[i]["gt_boxes"], infos[i]["gt_names"]) for i in ids]
        want = Y.assign_batch(tasks, coder, frames)
        got = {k: [v.cpu().numpy() for v in ex[k]] for k in KEYS}
        got["gt_overlap"] = np.concatenate(want["gt_overlap"])         # the loader does not hand it out
        _compare_to_restatement(got, want, coder, frames, anchors, f"loader batch {ids}")
        for t in range(6):
            assert got["labels"][t].shape == (len(ids), anchors[t].shape[0])
    assert sum(int((v > 0).sum()) for ex in batches for v in ex["labels"]) >= 15


def test_entry_refuses_bad_arguments_on_the_device_too():
    from al3d import lib
    so = lib.load()
    for what, args, word in Y.bad_argument_calls():
        assert so.al3d_assign_targets_f32(*args) == -1 and word in so.al3d_last_error(), what
    for what, args in Y.bad_launch_calls():
        assert so.al3d_assign_targets_launch_f32(*args) == -1, what
    plan = _plan(CASES[0]["tasks"], make_coder(CASES[0]))
    from al3d.detector_ops import assign_targets
    with pytest.raises(lib.Al3dError, match="float32"):
        assign_targets(plan, [np.zeros((1, 7))], gt_names=[["car"]])                 # float64 boxes
    with pytest.raises(lib.Al3dError, match="float32"):
        assign_targets(plan, [np.zeros((1, 9), np.float32)], gt_names=[["car"]])     # 9 columns for a 7-column coder
