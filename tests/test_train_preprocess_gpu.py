"""GPU suite of the train Preprocess (csrc/augment.hip behind datasets.augment, Preprocess(mode="train"), Voxelization's and
LoadPointCloudAnnotations' train branches, SweepDataset(mode="train")) against tests/golden/train_preprocess.npz, the output
of the reference's own functions (tools/gen_golden_train_preprocess.py).

Everything discrete is compared bit for bit: ``selected``, the drop mask, ``owner``, the kept counts, the row order after the
shuffle, and the boxes / names / classes after every stage (the boxes are host numpy through the reference's own calls).
Clouds: bit for bit when the per-object noise and the global rotation are zero -- ``(x - c) + c``, the flips, a rotation by
(cos, sin) = (1, 0) and one product with the scale are the same float32 operations on both sides.

The rotation bound (``train_preprocess_numpy.coord_bound``).  With rotation the reference multiplies through BLAS, whose
summation order and fused multiply-adds are not ours, so coordinates are held to a bound derived by counting roundings,
against a float64 chain on the same float32 inputs and float32 cos / sin.  One float32 rounding errs by at most u = 2^-24
of the rounded value.  With M = the largest |coordinate| of the input cloud, C the largest |centre coordinate|, L the
largest |loc noise| and D = M + C >= |p - c|:
  per-object step: one subtraction (u D), two products (u D each) and their sum (u sqrt2 D), the addition of c
  (u (sqrt2 D + C)) and of loc (u Mo, Mo = sqrt2 D + C + L the largest magnitude after the step); the subtraction's error
  passes through the rotation (at most sqrt2 times) -> e_obj = u (sqrt2 D + 2 D + sqrt2 D + (sqrt2 D + C) + Mo);
  global rotation: what came in, at most sqrt2 times, plus two products and a sum -> e_rot = sqrt2 e_obj + u (2 + sqrt2) Mo;
  scale s: e = s e_rot + u s sqrt2 Mo.
The kernel must be within e of the float64 chain and within 2 e of the golden (the reference errs by as much); the
untouched columns must be equal."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_preprocess_cases as TC  # noqa: E402
import train_preprocess_numpy as TN  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bits = TC.bits
NCASES = 11


@pytest.fixture(scope="module")
def database(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("train_db"))
    return root, TC.write_database(root)


def make_res(c, r, root):
    pts = torch.from_numpy(np.ascontiguousarray(c["points"])).to(DEV)
    return {"type": str(r["type"]), "mode": "train", "metadata": {"image_prefix": root, "num_point_features": 5}, "keep_debug": True,
            "lidar": {"points": pts, "combined": pts, "annotations": {"boxes": c["in_boxes"].copy(), "names": c["in_names"].copy()}}}


def snapshot(pre, res):
    d = pre._aug.last
    ann = res["lidar"]["annotations"]
    return dict(cloud=res["lidar"]["points"].cpu().numpy(), boxes=ann["gt_boxes"].copy(), names=np.array(ann["gt_names"]),
                classes=ann["gt_classes"].copy(), selected=np.asarray(d["selected"]).copy(),
                owner=d["owner"].cpu().numpy(), drop=None if d["drop_mask"] is None else d["drop_mask"].cpu().numpy().astype(bool),
                kept=int(d["kept"][0]), rows=d["rows"][0].copy(), stages=d["stages"][0], ns=int(d["sampled"][0]))


@pytest.fixture(scope="module")
def replayed(database):
    """Every case through Preprocess(train) with the recorded draws fed back -> {case: snapshot}."""
    from al3d.datasets import Preprocess
    root, pkls = database
    out = {}
    for ri in range(TC.num_runs()):
        ids = TC.cases_of(ri)
        with TN.ReplayRandom(TC.case(ids[0])["init_log"]):
            pre = Preprocess(cfg=TC.train_cfg(ri, pkls), device=DEV)
        for ci in ids:
            c = TC.case(ci)
            res = make_res(c, TC.run(ri), root)
            with TN.ReplayRandom(c["log"]):
                res, _ = pre(res, None)
            out[ci] = snapshot(pre, res)
    return out


def check_discrete(c, h, got):
    assert np.array_equal(got["selected"], c["selected"]), "selected"
    keep = TC.kept_mask(c, h)
    if got["drop"] is None:
        assert not c["drop"].any()
    else:
        assert np.array_equal(got["drop"][h["ns"]:], c["drop"].astype(bool)) and not got["drop"][:h["ns"]].any(), "drop mask"
    assert got["ns"] == h["ns"]
    assert np.array_equal(got["owner"][keep], c["owner"]), "owner"
    assert got["kept"] == len(c["cloud"]) == int(keep.sum()), "kept count"
    assert np.array_equal(got["rows"][h["perm"]], np.arange(len(h["perm"]))), "row order after the shuffle"
    for key, want in (("noise", c["boxes_noise"]), ("flip", c["boxes_flip"]), ("rot", c["boxes_rot"])):
        assert got["stages"][key].shape == want.shape and np.array_equal(bits(got["stages"][key]), bits(want)), f"boxes after {key}"
    assert np.array_equal(bits(got["boxes"]), bits(c["boxes_scale"])) and np.array_equal(bits(got["boxes"]), bits(c["final_boxes"]))
    assert got["boxes"].dtype == c["final_boxes"].dtype
    assert np.array_equal(got["names"], c["final_names"]) and np.array_equal(got["classes"], c["final_classes"])
    assert got["classes"].dtype == np.int32


def check_cloud(c, r, h, got):
    cloud = got["cloud"]
    assert cloud.shape == c["cloud"].shape and cloud.dtype == np.float32
    assert np.array_equal(bits(cloud[:, 3:]), bits(c["cloud"][:, 3:])), "untouched columns"
    zero = not np.any(r["gt_loc_noise"]) and not np.any(r["gt_rot_noise"]) and not np.any(r["global_rot_noise"])
    if zero:
        assert np.array_equal(bits(cloud), bits(c["cloud"])), "zero noise and zero rotation: the cloud is the reference's, bit for bit"
        return
    chain, _, _ = TN.augment_points_np(h["cloud"], h["ns"], h["planes"], h["mask"], h["boxes"][:, :3], h["cos"], h["sin"], h["loc"],
                                       c["selected"], h["flip"], np.cos(h["angle"]), np.sin(h["angle"]), h["scale"],
                                       bool(r["symmetry"]), drop_planes=h["drop_planes"], perm=h["perm"], dtype=np.float64)
    bound = TN.coord_bound(h["cloud"], h["boxes"][:, :3], h["loc"], h["scale"])
    e_chain = np.abs(cloud[:, :3].astype(np.float64) - chain[:, :3]).max()
    e_gold = np.abs(cloud[:, :3].astype(np.float64) - c["cloud"][:, :3]).max()
    print(f"bound {bound:.3e}: kernel - float64 chain {e_chain:.3e}, kernel - golden {e_gold:.3e}")
    assert e_chain <= bound and e_gold <= 2 * bound


@pytest.mark.parametrize("ci", range(NCASES))
def test_recorded_draws_reproduce_the_reference(replayed, ci):
    """Items 3-5: selected, drop mask, owner, kept count, shuffle order and the boxes after every stage bit for bit; the
    cloud bit for bit without rotation, inside the derived bound with it."""
    c = TC.case(ci)
    r = TC.run(c["run"])
    h = TC.host_inputs(c, r)
    check_discrete(c, h, replayed[ci])
    check_cloud(c, r, h, replayed[ci])


def test_golden_has_the_cases(replayed):
    """0 boxes, more than 64 boxes, 7 and 9 columns, a failed box that still owns points, a later try, both drop settings."""
    sizes = [len(TC.case(ci)["selected"]) for ci in range(NCASES)]
    assert min(sizes) >= 0 and max(sizes) > 64 and any(len(TC.case(ci)["in_boxes"]) == 0 for ci in range(NCASES))
    assert {int(TC.run(ri)["cols"]) for ri in range(TC.num_runs())} == {7, 9}
    assert any((TC.case(ci)["selected"] > 0).any() for ci in range(NCASES))
    d = TC.case(NCASES - 1)
    assert d["selected"][1] == -1 and (d["owner"] == 1).any()
    assert any(replayed[ci]["drop"] is not None and replayed[ci]["drop"].any() for ci in range(NCASES))


@pytest.mark.parametrize("ri", range(4))
def test_seeded_preprocess_consumes_numpy_like_the_reference(database, replayed, ri):
    """Item 6: with np.random seeded as stored, Preprocess(train) draws for itself and leaves ``np.random.get_state()`` where
    the reference left it, after the constructor and after every call; the outputs are those of the replayed run."""
    from al3d.datasets import Preprocess
    root, pkls = database
    ids = TC.cases_of(ri)
    np.random.seed(TC.case(ids[0])["seed"])
    pre = Preprocess(cfg=TC.train_cfg(ri, pkls), device=DEV)
    assert TN.state_digest() == str(TC.case(ids[0])["init_digest"])
    for ci in ids:
        c = TC.case(ci)
        res, _ = pre(make_res(c, TC.run(ri), root), None)
        assert TN.state_digest() == str(c["digest"]), f"case {ci}: np.random is not where the reference left it"
        got = snapshot(pre, res)
        for k in ("cloud", "boxes", "selected", "owner", "rows", "classes"):
            assert np.array_equal(bits(got[k]), bits(replayed[ci][k])), k


# ---- the entries alone: launch shapes, sizes the golden lacks, bad input --------------------------------------------------
def dev_inputs(h):
    from al3d.datasets.augment import _up
    d = dict(points=_up(h["cloud"], np.float32, DEV), planes=_up(h["planes"], np.float32, DEV), valid=_up(h["mask"], np.uint8, DEV),
             centres3=_up(h["boxes"][:, :3], np.float32, DEV), centres2=_up(h["boxes"][:, :2], np.float32, DEV),
             corners=_up(h["corners"], np.float32, DEV), cos=_up(h["cos"], np.float32, DEV), sin=_up(h["sin"], np.float32, DEV),
             loc=_up(h["loc"], np.float64, DEV), box_off=torch.tensor([0, len(h["boxes"])], dtype=torch.int32, device=DEV),
             point_off=torch.tensor([0, len(h["cloud"])], dtype=torch.int64, device=DEV),
             sampled_off=torch.tensor([h["ns"]], dtype=torch.int64, device=DEV))
    if h["drop_planes"] is not None:
        d["drop_planes"] = _up(h["drop_planes"], np.float32, DEV)
        d["drop_off"] = torch.tensor([0, len(h["drop_planes"])], dtype=torch.int32, device=DEV)
    return d


def run_entries(h, d, symmetry, launch):
    """noise, count, points with one launch shape -> host arrays."""
    from al3d.datasets import augment as A
    sel, st = A.noise_per_box_device(d["corners"], d["centres2"], d["valid"], d["cos"], d["sin"], d["loc"], d["box_off"], launch)
    assert st.item() == 0
    drop = ws = None
    n = len(h["cloud"])
    if "drop_planes" in d:
        drop, kept, ws, st = A.augment_points_count(d["points"], d["point_off"], d["sampled_off"], d["drop_planes"], d["drop_off"], launch)
        assert st.item() == 0
        n = int(kept.item())
    inv = np.empty(n, dtype=np.int32)
    perm = h["perm"] if len(h["perm"]) == n else np.arange(n)[::-1]
    inv[perm] = np.arange(n, dtype=np.int32)
    out_off = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    xf = torch.tensor([[np.float32(np.cos(h["angle"])), np.float32(np.sin(h["angle"])), np.float32(h["scale"])]], device=DEV)
    flip = torch.tensor([[int(h["flip"][0]), int(h["flip"][1])]], dtype=torch.uint8, device=DEV)
    out, owner, st = A.augment_points(d["points"], d["point_off"], out_off, n, xf, drop_mask=drop, workspace=ws, planes=d["planes"],
                                      box_off=d["box_off"], valid=d["valid"], centres=d["centres3"], rot_cos=d["cos"],
                                      rot_sin=d["sin"], loc=d["loc"], selected=sel, flip=flip, symmetry=symmetry,
                                      rows=torch.from_numpy(inv).to(DEV), want_owner=True, launch=launch)
    assert st.item() == 0
    return dict(selected=sel.cpu().numpy(), out=out.cpu().numpy(), owner=owner.cpu().numpy(),
                drop=np.zeros(len(h["cloud"]), bool) if drop is None else drop.cpu().numpy().astype(bool))


SHAPES = [(g, t, tile) for g in (1, 7, 32) for t in (64, 128, 256) for tile in (1, 64)]


@pytest.mark.parametrize("ci", [0, 6])
def test_every_launch_shape_gives_the_same_bytes(ci):
    """Item 7 on a noisy case with drops (case 0) and on the 73-box frame (case 6: two LDS tiles at tile 64)."""
    c = TC.case(ci)
    h = TC.host_inputs(c, TC.run(c["run"]))
    d = dev_inputs(h)
    want = run_entries(h, d, False, None)
    assert np.array_equal(want["selected"], c["selected"])
    for shape in SHAPES:
        got = run_entries(h, d, False, shape)
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), f"launch shape {shape}: {k} differs"


def test_sizes_the_golden_lacks_equal_the_restatement():
    """P = 70001 points, R = 130 boxes, T = 100 tries, 5000 sampled points, 30 drop boxes, against the numpy restatement:
    discrete outputs exact, coordinates inside the derived bound of the float64 chain."""
    from al3d.datasets.augment import box2d_to_corner
    from al3d.detector_ops import box_planes
    rng = np.random.default_rng(77)
    P, R, T, ns = 70001, 130, 100, 5000
    b = np.zeros((R, 9), dtype=np.float32)
    b[:, :2], b[:, 2] = rng.uniform(-40, 40, (R, 2)), rng.uniform(-1.5, 0.5, R)
    b[:, 3:6] = rng.uniform([1.0, 2.0, 1.2], [3.5, 8.0, 3.0], (R, 3))
    b[:, 6], b[:, 8] = rng.uniform(-1.5, 1.5, R), rng.uniform(-3, 3, R)
    pts = np.zeros((P, 5), dtype=np.float32)
    pts[:, :2], pts[:, 2] = rng.uniform(-42, 42, (P, 2)), rng.uniform(-2, 1, P)
    pick = rng.integers(0, R, P // 3)                                      # a third of the points sit near box centres
    pts[:P // 3, :3] = b[pick, :3] + rng.normal(0, 0.6, (P // 3, 3)).astype(np.float32)
    pts[:, 3], pts[:, 4] = rng.integers(0, 256, P), rng.uniform(0, 0.5, P)
    rot, loc = rng.uniform(-0.3, 0.3, (R, T)), rng.normal(0, 0.3, (R, T, 3))
    mask = rng.uniform(size=R) < 0.8
    h = dict(boxes=b, mask=mask, ns=ns, cloud=pts, drop_planes=box_planes(np.ascontiguousarray(b[100:])), loc=loc, rot=rot,
             cos=np.cos(rot).astype(np.float32), sin=np.sin(rot).astype(np.float32), corners=box2d_to_corner(b[:, [0, 1, 3, 4, 6]]),
             flip=[True, True], angle=0.31, scale=1.03, perm=np.zeros(0, np.int64), planes=box_planes(np.ascontiguousarray(b[:, :7])))
    d = dev_inputs(h)
    got = run_entries(h, d, True, None)
    sel = TN.noise_per_box_np(h["corners"], b[:, :2], mask, h["cos"], h["sin"], loc)
    assert np.array_equal(got["selected"], sel) and (sel > 0).any() and (sel == 0).any()
    n = int((~got["drop"]).sum())
    perm = np.arange(n)[::-1]
    args = (pts, ns, h["planes"], mask, b[:, :3], h["cos"], h["sin"], loc, sel, h["flip"], np.cos(0.31), np.sin(0.31), 1.03, True)
    out, owner, drop = TN.augment_points_np(*args, drop_planes=h["drop_planes"], perm=perm)
    assert np.array_equal(got["drop"], drop) and drop.any() and np.array_equal(got["owner"], owner) and (owner >= 0).sum() > 1000
    assert got["out"].shape == out.shape and np.array_equal(bits(got["out"][:, 3:]), bits(out[:, 3:]))
    chain, _, _ = TN.augment_points_np(*args, drop_planes=h["drop_planes"], perm=perm, dtype=np.float64)
    bound = TN.coord_bound(pts, b[:, :3], loc, 1.03)
    err = np.abs(got["out"][:, :3].astype(np.float64) - chain[:, :3]).max()
    print(f"bound {bound:.3e}: kernel - float64 chain {err:.3e}; bitwise equal to the float32 restatement: "
          f"{np.array_equal(bits(got['out']), bits(out))}")
    assert err <= bound
    for shape in [(1, 64, 1), (7, 128, 64)]:
        other = run_entries(h, d, True, shape)
        for k in got:
            assert other[k].tobytes() == got[k].tobytes(), f"launch shape {shape}: {k} differs"


def test_limits_and_bad_offsets_set_their_bit_and_write_nothing():
    """Item 8: too many boxes, a bad try count, descending offsets, a sampled count beyond the frame, rows outside the frame
    and a workspace of another launch shape."""
    from al3d import lib
    from al3d.datasets import augment as A
    i32 = dict(dtype=torch.int32, device=DEV)

    def noise(R, T, box_off):
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)  # noqa: E731
        sel, st = torch.full((R,), 77, **i32), torch.zeros(1, **i32)
        lib.call("al3d_noise_per_box_launch_f32", z(R, 4, 2).data_ptr(), z(R, 2).data_ptr(), torch.ones(R, dtype=torch.uint8, device=DEV).data_ptr(),
                 z(R, max(T, 1)).data_ptr(), z(R, max(T, 1)).data_ptr(), z(R, max(T, 1), 3, dt=torch.float64).data_ptr(),
                 torch.tensor(box_off, **i32).data_ptr(), len(box_off) - 1, R, T, sel.data_ptr(), st.data_ptr(), 1, 64, 4,
                 torch.cuda.current_stream().cuda_stream)
        return sel.cpu().numpy(), st.item()

    sel, st = noise(1025, 4, [0, 1025])
    assert st == 32 and (sel == 77).all()
    sel, st = noise(4, 257, [0, 4])
    assert st == 64 and (sel == 77).all()
    sel, st = noise(4, 0, [0, 4])
    assert st == 64 and (sel == 77).all()
    sel, st = noise(6, 4, [0, 4, 2, 2])                                    # frame 1 descends: empty; frame 0 runs
    assert st == 2 and (sel[:4] != 77).all() and (sel[4:] == 77).all()

    pts = torch.rand(300, 5, device=DEV)
    off = lambda *v: torch.tensor(v, dtype=torch.int64, device=DEV)        # noqa: E731
    planes = torch.zeros(0, 6, 4, device=DEV)
    xf = torch.tensor([[1.0, 0.0, 1.0], [1.0, 0.0, 1.0]], device=DEV)
    # count: frame 0 has a sampled count beyond its size, frame 1 is fine
    drop, kept, ws, st = A.augment_points_count(pts, off(0, 100, 300), off(101, 0), planes, torch.zeros(3, **i32))
    assert st.item() == 128 and kept.cpu().tolist() == [0, 200]
    # points: descending point_off of frame 1 -> nothing of it is written
    out = torch.full((300, 5), -7.0, device=DEV)
    _, _, st = A.augment_points(pts, off(0, 100, 50), off(0, 100, 100), 300, xf, out=out)
    assert st.item() == 1 and torch.equal(out[:100], pts[:100]) and (out[100:] == -7).all()
    # rows outside the frame are not written
    rows = torch.arange(100, **i32)
    rows[3], rows[50] = 100, -1
    out = torch.full((100, 5), -7.0, device=DEV)
    _, _, st = A.augment_points(pts[:100].contiguous(), off(0, 100), off(0, 100), 100, xf[:1], rows=rows, out=out)
    assert st.item() == 16 and (out[3] == -7).all() and (out[50] == -7).all() and int((out[:, 0] == -7).sum()) == 2
    hit = torch.ones(100, dtype=torch.bool)
    hit[[3, 50]] = False
    assert torch.equal(out.cpu()[hit], pts[:100].cpu()[hit])
    # a workspace counted with another launch shape
    drop, kept, ws, st = A.augment_points_count(pts, off(0, 300), off(0), planes, torch.zeros(2, **i32), launch=(7, 128, 64))
    out = torch.full((300, 5), -7.0, device=DEV)
    _, _, st = A.augment_points(pts, off(0, 300), off(0, 300), 300, xf[:1], drop_mask=drop, workspace=ws, out=out, launch=(32, 256, 64))
    assert st.item() == 8 and (out == -7).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def assigner_cfg():
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(TC.ROOT, "examples", "active", "cbgs_spatial_temporal_feature.py"))
    gens = {g["class_name"]: dict(g) for g in cfg.target_assigner.anchor_generators}
    tasks = [dict(num_class=2, class_names=["car", "pedestrian"]), dict(num_class=2, class_names=["truck", "traffic_cone"])]
    ta = dict(cfg.target_assigner, tasks=tasks, anchor_generators=[gens[n] for t in tasks for n in t["class_names"]])
    return dict(box_coder=cfg.box_coder, target_assigner=ta, out_size_factor=8, debug=False)


def test_train_pipeline_end_to_end(database, tmp_path):
    """Item 9: files -> LoadPointCloudFromFile -> LoadPointCloudAnnotations -> Preprocess(train) -> Voxelization -> AssignTarget
    -> Reformat through SweepDataset(mode="train"), run C's config and draws, on the on-disk pool with a database built by
    create_groundtruth_database: the annotations after the range filter are the golden's, and labels / reg_targets /
    reg_weights are AssignTarget's on the golden's final boxes."""
    import pickle
    from al3d.datasets import AssignTarget, Compose, SweepDataset, create_groundtruth_database
    g = TC.golden()
    root = str(tmp_path)
    infos = TC.write_pool(root)
    nsw, suffix = int(g["nsweeps"]), str(g["suffix"])
    info_path = os.path.join(root, f"infos_train_{nsw:02d}sweeps_withvelo_{suffix}.pkl")
    with open(info_path, "wb") as f:
        pickle.dump([infos[i] for i in g["db_frames"]], f)
    with TN.ReplayRandom([]):                                              # the loader's sweep order: list order
        create_groundtruth_database("NUSC", root, info_path, nsweeps=nsw, suffix=suffix)
    db_pkl = os.path.join(root, f"dbinfos_train_{nsw}sweeps_withvelo_{suffix}.pkl")
    ri = 2
    cfg = TC.train_cfg(ri, (db_pkl, None))
    rng = [float(v) for v in g["range"]]
    vox = dict(range=rng, voxel_size=[0.25, 0.25, 8.0], max_points_in_voxel=5, max_voxel_num=20000)
    acfg = assigner_cfg()
    ids = TC.cases_of(ri)
    with TN.ReplayRandom(TC.case(ids[0])["init_log"]):
        pipe = Compose([dict(type="LoadPointCloudFromFile", dataset="NuScenesDataset", device=DEV),
                        dict(type="LoadPointCloudAnnotations", with_bbox=True), dict(type="Preprocess", cfg=cfg, device=DEV),
                        dict(type="Voxelization", cfg=vox, device=DEV), dict(type="AssignTarget", cfg=acfg, device=DEV),
                        dict(type="Reformat")])
    ds = SweepDataset([infos[i] for i in g["train_frames"]], pipe, nsweeps=nsw, mode="train", root_path=root)
    stage = AssignTarget(cfg=acfg, device=DEV)
    for ci in ids:
        c = TC.case(ci)
        with TN.ReplayRandom(c["log"]):
            ex = ds[list(g["train_frames"]).index(c["frame"])]
        m = c["range_mask"].astype(bool)
        assert ex["points"].shape == c["cloud"].shape and np.array_equal(bits(ex["points"].cpu().numpy()), bits(c["cloud"]))
        res = dict(mode="train", lidar=dict(voxels=dict(shape=ex["shape"]), annotations=dict(
            gt_boxes=c["final_boxes"][m].copy(), gt_classes=c["final_classes"][m].copy(), gt_names=c["final_names"][m].copy())))
        want = stage(res, {})[0]["lidar"]["targets"]
        for k in ("labels", "reg_targets", "reg_weights"):
            assert len(ex[k]) == len(want[k]) == 2
            for a, b in zip(ex[k], want[k]):
                assert torch.equal(a, b), k
        assert sum(int((v > 0).sum()) for v in ex["labels"]) > 0 or not m.any()


def test_file_loader_with_train_cfg_gives_the_same_batch(tmp_path):
    """Item 9, the loader: FileSweepLoader(with_targets=True, train_cfg=...) with batches of one frame and the same draws
    yields the golden's cloud and annotations after the range filter, and AssignTarget's targets on them."""
    from al3d.datasets import AssignTarget, FileSweepLoader
    g = TC.golden()
    root = str(tmp_path)
    infos = TC.write_pool(root)
    pkls = TC.write_database(root)
    ri = 2
    ids = TC.cases_of(ri)
    vox = dict(range=[float(v) for v in g["range"]], voxel_size=[0.25, 0.25, 8.0], max_points_in_voxel=5, max_voxel_num=20000)
    acfg = assigner_cfg()
    order = [TC.case(ci)["frame"] for ci in ids]
    with TN.ReplayRandom(TC.case(ids[0])["init_log"]):
        loader = FileSweepLoader(infos, vox, None, batch_size=1, device=DEV, nsweeps=int(g["nsweeps"]), root=root, indices=order,
                                 with_targets=True, target_cfg=acfg, train_cfg=TC.train_cfg(ri, pkls))
    stage = AssignTarget(cfg=acfg, device=DEV)
    it = iter(loader)
    for ci in ids:
        c = TC.case(ci)
        with TN.ReplayRandom(c["log"]):
            ex = next(it)
        m = c["range_mask"].astype(bool)
        n = int(ex["point_offsets"][-1])
        assert n == len(c["cloud"]) and np.array_equal(bits(ex["points"][:n].cpu().numpy()), bits(c["cloud"]))
        assert np.array_equal(bits(ex["gt_boxes"][0]), bits(c["final_boxes"][m])) and np.array_equal(ex["gt_names"][0], c["final_names"][m])
        res = dict(mode="train", lidar=dict(voxels=dict(shape=ex["shape"][0]), annotations=dict(
            gt_boxes=c["final_boxes"][m].copy(), gt_classes=c["final_classes"][m].copy(), gt_names=c["final_names"][m].copy())))
        want = stage(res, {})[0]["lidar"]["targets"]
        for k in ("labels", "reg_targets", "reg_weights"):
            for a, b in zip(ex[k], want[k]):
                assert torch.equal(a.reshape(b.shape), b), k
    assert next(it, None) is None


def test_val_mode_is_unchanged():
    """Item 10: Preprocess(val) passes the combined cloud on and touches no annotation; the annotations loader is a
    pass-through outside train mode."""
    from al3d.datasets import LoadPointCloudAnnotations, Preprocess
    pts = torch.rand(50, 5, device=DEV)
    res = {"type": "NuScenesDataset", "mode": "val", "lidar": {"points": pts[:, :4], "combined": pts, "annotations": None}}
    info = dict(gt_boxes=np.zeros((2, 9)), gt_names=np.array(["car", "car"]))
    res, _ = LoadPointCloudAnnotations()(res, info)
    assert res["lidar"]["annotations"] is None
    res, _ = Preprocess(cfg=dict(mode="val", shuffle_points=False))(res, info)
    assert res["lidar"]["points"] is pts and res["mode"] == "val" and res["lidar"]["annotations"] is None
