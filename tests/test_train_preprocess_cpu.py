"""CPU suite of the train Preprocess: the host sampler and the numpy restatement against
tests/golden/train_preprocess.npz (the reference's own Preprocess / DataBaseSamplerV2 / noise_per_object_v3_ /
box_collision_test / filter_gt_box_outside_range, tools/gen_golden_train_preprocess.py), the shuffle rule, and the keys that
are refused by name.

Coordinates of the restatement are held to the bound derived in tests/test_train_preprocess_gpu.py (``TN.coord_bound``);
everything discrete is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_preprocess_cases as TC  # noqa: E402
import train_preprocess_numpy as TN  # noqa: E402


@pytest.fixture(scope="module")
def database(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("train_db"))
    return root, TC.write_database(root)


bits, host_inputs, kept_mask = TC.bits, TC.host_inputs, TC.kept_mask


@pytest.mark.parametrize("ri", range(4))
def test_host_sampler_equals_the_reference_bit_for_bit(database, ri):
    """names, boxes, points, masks, group ids of every ``sample_all`` call, the ``None`` returns included, with the batch
    samplers' shuffles replayed; seeded, building the sampler leaves ``np.random`` where the reference left it."""
    from al3d.datasets.db_sampler import build_dbsampler
    root, pkls = database
    cfg = TC.train_cfg(ri, pkls)["db_sampler"]
    ids = TC.cases_of(ri)
    first = TC.case(ids[0])
    np.random.seed(first["seed"])
    build_dbsampler(cfg)
    assert TN.state_digest() == str(first["init_digest"])
    with TN.ReplayRandom(first["init_log"]):
        sampler = build_dbsampler(cfg)
    for ci in ids:
        c = TC.case(ci)
        with TN.ReplayRandom(TC.sampler_log(c["log"])):
            sd = sampler.sample_all(root, c["in_boxes"], c["in_names"], 5, False, gt_group_ids=None, calib=None)
        assert (sd is not None) == bool(c["has_sample"])
        if sd is None:
            continue
        assert list(sd.keys()) == ["gt_names", "difficulty", "gt_boxes", "points", "gt_masks", "group_ids"]
        for k in ("gt_names", "difficulty", "gt_boxes", "points", "gt_masks", "group_ids"):
            want = c[f"sample_{k}"]
            assert sd[k].shape == want.shape and sd[k].dtype == want.dtype, k
            assert np.array_equal(bits(sd[k]), bits(want)), k


def test_golden_covers_every_sampler_rule():
    events = set()
    for ci in range(TC.num_cases()):
        events |= set(str(e) for e in TC.case(ci)["events"])
    assert events >= {"wrap", "hits_gt", "hits_earlier_class", "freed_by_rejection", "nonpositive", "none"}


@pytest.mark.parametrize("ci", range(11))
def test_numpy_restatement_equals_the_golden(ci):
    c = TC.case(ci)
    r = TC.run(c["run"])
    h = host_inputs(c, r)
    zero = not np.any(r["gt_loc_noise"]) and not np.any(r["gt_rot_noise"])
    sel = TN.noise_per_box_np(h["corners"], h["boxes"][:, :2], h["mask"], h["cos"], h["sin"], h["loc"])
    assert np.array_equal(sel, c["selected"])
    out, owner, drop = TN.augment_points_np(h["cloud"], h["ns"], h["planes"], h["mask"], h["boxes"][:, :3], h["cos"], h["sin"],
                                            h["loc"], sel, h["flip"], np.cos(h["angle"]), np.sin(h["angle"]), h["scale"],
                                            bool(r["symmetry"]), drop_planes=h["drop_planes"], perm=h["perm"])
    assert np.array_equal(drop[h["ns"]:], c["drop"].astype(bool)) and not drop[:h["ns"]].any()
    assert np.array_equal(owner[kept_mask(c, h)], c["owner"]) or len(c["owner"]) == 0
    assert out.shape == c["cloud"].shape
    assert np.array_equal(bits(out[:, 3:]), bits(c["cloud"][:, 3:]))
    if zero and not np.any(r["global_rot_noise"]):
        assert np.array_equal(bits(out), bits(c["cloud"]))
    else:
        bound = TN.coord_bound(h["cloud"], h["boxes"][:, :3], h["loc"], h["scale"])
        assert np.abs(out[:, :3].astype(np.float64) - c["cloud"][:, :3]).max() <= 2 * bound


@pytest.mark.parametrize("n", [0, 1, 2, 1000, 70001])
def test_index_shuffle_equals_row_shuffle(n):
    """``np.random.shuffle`` on an index array of length n draws what it draws on the [n, 5] rows: the device applies the
    index form."""
    rows = np.arange(n * 5, dtype=np.float32).reshape(n, 5)
    np.random.seed(1234 + n)
    st = np.random.get_state()
    idx = np.arange(n)
    np.random.shuffle(idx)
    after_idx = TN.state_digest()
    np.random.set_state(st)
    shuffled = rows.copy()
    np.random.shuffle(shuffled)
    assert TN.state_digest() == after_idx
    assert np.array_equal(rows[idx], shuffled)


def test_collision_mirror_equals_the_restatement():
    """datasets.augment.box_collision_test against the one-vs-all restatement on crossing, contained, touching-free and far
    boxes, in float32."""
    from al3d.datasets.augment import box2d_to_corner, box_collision_test
    rng = np.random.default_rng(5)
    b = np.concatenate([rng.uniform(-20, 20, (40, 2)), rng.uniform(0.5, 4, (40, 2)), rng.uniform(-3, 3, (40, 1))], 1).astype(np.float32)
    b[1] = [b[0, 0] + 0.1, b[0, 1], 0.2, 0.2, 0.4]                         # inside box 0 when box 0 is large
    b[0, 2:4] = [5.0, 5.0]
    corners = box2d_to_corner(b)
    got = box_collision_test(corners, corners)
    want = np.stack([TN.collide_one_vs_all(corners[i], corners) for i in range(len(b))])
    assert np.array_equal(got, want)
    assert got[0, 1] and got[1, 0] and not got.diagonal().any() and got.any(1).sum() > 10 and (~got.any(1)).sum() >= 1


@pytest.mark.parametrize("ci", range(11))
def test_range_filter_equals_the_golden(ci):
    from al3d.datasets.augment import filter_gt_box_outside_range
    c = TC.case(ci)
    rng = np.array(TC.golden()["range"], dtype=np.float32)[[0, 1, 3, 4]]
    if len(c["final_boxes"]):
        assert np.array_equal(filter_gt_box_outside_range(c["final_boxes"], rng), c["range_mask"])


def test_status_bits_mirror_the_header():
    import re
    from al3d.datasets import augment
    hdr = open(os.path.join(TC.ROOT, "include", "al3d.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (AL3D_AUG_[A-Z_]+) (\d+)", hdr)}
    bits_ = {v for k, v in defs.items() if k.startswith(("AL3D_AUG_BAD", "AL3D_AUG_TOO", "AL3D_AUG_FRAME"))}
    assert bits_ == set(augment.AUG_STATUS)
    assert (defs["AL3D_AUG_MAX_BOXES"], defs["AL3D_AUG_MAX_TRIES"]) == (augment.AUG_MAX_BOXES, augment.AUG_MAX_TRIES)
    assert (defs["AL3D_AUG_GROUPS"], defs["AL3D_AUG_THREADS"], defs["AL3D_AUG_NOISE_TILE"]) == \
        (augment.AUG_GROUPS, augment.AUG_THREADS, augment.AUG_NOISE_TILE)


@pytest.mark.parametrize("key,value", [("random_crop", True), ("add_rgb_to_points", True), ("reference_detections", [1]),
                                       ("remove_outside_points", True), ("remove_environment", True), ("random_select", True),
                                       ("npoints", 1000), ("global_rot_per_obj_range", [-0.5, 0.5])])
def test_out_of_scope_keys_raise_by_name(database, key, value):
    from al3d.datasets import Preprocess
    cfg = TC.train_cfg(0, database[1])
    cfg[key] = value
    with pytest.raises(NotImplementedError, match=key):
        Preprocess(cfg=cfg)


def test_out_of_scope_sampler_keys_raise_by_name(database):
    from al3d.datasets.db_sampler import build_dbsampler
    cfg = TC.train_cfg(0, database[1])["db_sampler"]
    with pytest.raises(NotImplementedError, match="sample_groups"):
        build_dbsampler(dict(cfg, sample_groups=[dict(car=2, truck=1)]))
    with pytest.raises(NotImplementedError, match="global_random_rotation_range_per_object"):
        build_dbsampler(dict(cfg, global_random_rotation_range_per_object=[-0.5, 0.5]))
    s = build_dbsampler(cfg)
    with pytest.raises(NotImplementedError, match="gt_group_ids"):
        s.sample_all(database[0], np.zeros((0, 9), np.float32), np.array([]), 5, gt_group_ids=np.zeros(0))
    with pytest.raises(NotImplementedError, match="random_crop"):
        s.sample_all(database[0], np.zeros((0, 9), np.float32), np.array([]), 5, random_crop=True)
