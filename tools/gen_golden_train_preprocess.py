#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Golden vectors for the train Preprocess -> tests/golden/train_preprocess.npz.

Runs the reference's own, unmodified ``Preprocess.__call__`` (det3d/datasets/pipelines/preprocess.py:57-256),
``DataBaseSamplerV2`` (det3d/core/sampler/sample_ops.py), ``noise_per_object_v3_``, ``box_collision_test`` and
``filter_gt_box_outside_range`` (det3d/core/sampler/preprocess.py) on a synthetic on-disk pool of 6 frames (key file + 2 of 3
listed sweeps each, <= ~2,000 merged points): frames 0-2 are augmented (70 boxes in frame 0 so the kernels' 64-box tile is
crossed, 0 boxes in frame 1, 14 in frame 2), frames 3-5 only feed the reference's ``create_groundtruth_database``.  The two
halves are separate on purpose: an object sampled into its own frame is the SAME box twice, every comparison of the
collision test is then an exact tie, and a tie has no margin.  Needs the reference tree (build container only).

Stand-ins, none with algorithmic content (oracle/ref_import.py and tools/gen_golden_gt_database.py have the rest: no numba,
so the ``njit`` functions run as the python they are, on numpy float32 scalars):

* ``det3d.builder`` is a local module whose ``build_dbsampler`` opens the pickle and hands the config's values to the
  reference's own ``DataBaseSamplerV2`` / ``DataBasePreprocessor`` / ``DBFilterBy*`` (the real module imports the model
  zoo); ``bbox_overlaps``, ``VoxelGenerator`` and ``TargetAssigner`` are names ``pipelines/preprocess.py`` imports and the train
  branch of ``Preprocess`` never calls; ``kitti_common.drop_arrays_by_name`` is the reference's own function, compiled from
  its source lines alone (the module needs skimage at import);
* ``box_collision_test`` is re-compiled from its own source with ``x is True`` / ``x is False`` turned into ``x == True`` /
  ``x == False``: numba compiles ``is`` on a boolean as a comparison of values, plain python compares identities, and a
  numpy bool_ is never the ``True`` object -- as plain python the function would skip its two containment tests.  Nothing
  else of it changes;
* ``np.random`` is wrapped by a recorder (tests/train_preprocess_numpy.py): every draw is stored, the loader's sweep order
  (``choice(n, k)``) is pinned to list order, and a 2-D shuffle is stored as the index permutation it applied (asserted equal
  to the row shuffle under the same state).

Stored: arrays and strings only.  The pool's raw files and infos, the database files and dbinfos (9-column, and a 7-column
copy with the velocity columns removed for the KittiDataset-typed run), and per case: the seed, the config, the recorded
draws, the ``sample_all`` dict, ``selected``, owners, the drop mask, the boxes after every stage, the range-filter mask, the
final cloud and a digest of ``np.random.get_state()`` after the call.

Margins.  In float64 every comparison ``a > b`` / ``cross >= 0`` that ``box_collision_test`` evaluates has
``|a - b| > 1e-4 (|a| + |b|)``, and every (point, box) pair has the sign margin of tools/gen_golden_gt_database.py.  A scene
point that fails is redrawn in its raw file (the share is printed; more than 1 % stops the script).  A case whose collision
comparisons or sampled points fail takes the next seed (seeds are not inputs; the count is printed); run A also takes the
next seed until its four cases show all four flip outcomes and both noise events (seeds tried: printed).  The zero-noise runs are
exempt from the collision margin: a try there is the box itself, exact by construction."""
import ast
import importlib
import inspect
import logging
import os
import pickle
import shutil
import sys
import tempfile
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import ref_import as R  # noqa: E402
import gen_golden_gt_database as G  # noqa: E402
import train_preprocess_numpy as TN  # noqa: E402

NSWEEPS, SUFFIX = 3, "g"
CLASSES = G.CLASSES                                                       # car, pedestrian, truck, traffic_cone
TRAIN, DB = [0, 1, 2], [3, 4, 5]
NBOX = {0: (int(os.environ.get("AL3D_GOLDEN_F0_BOXES", 70)), 1), 1: (0, 0), 2: (14, 0), 3: (40, 1), 4: (22, 0), 5: (14, 1)}
RANGE = [-16.0, -16.0, -5.0, 16.0, 16.0, 3.0]                             # Voxelization's: some boxes leave it

PREP = [dict(filter_by_min_num_points=dict(car=2, pedestrian=2, truck=2, traffic_cone=2)), dict(filter_by_difficulty=[-1])]
NOISY = dict(gt_rot_noise=[-0.3, 0.3], gt_loc_noise=[0.4, 0.4, 0.1], global_rot_noise=[-0.3925, 0.3925])
ZERO = dict(gt_rot_noise=[0.0, 0.0], gt_loc_noise=[0.0, 0.0, 0.0], global_rot_noise=[0.0, 0.0])
RUNS = [
    # the noisy runs are small on purpose: every evaluated comparison needs its margin, and a box that never finds a free try
    # evaluates 100 x (boxes - 1) of them
    dict(name="A", type="NuScenesDataset", cols=9, remove=True, symmetry=False, noise=NOISY, frames=[2, 1, 2, 1], boxes=(2, None),
         class_names=["car", "pedestrian", "truck"],
         groups=[dict(car=6), dict(pedestrian=7), dict(truck=4), dict(traffic_cone=0)]),
    dict(name="B", type="KittiDataset", cols=7, remove=False, symmetry=True, noise=ZERO, frames=[0, 1, 2],
         class_names=["car", "pedestrian", "truck"], groups=[dict(car=20), dict(pedestrian=6), dict(truck=2)]),
    dict(name="C", type="NuScenesDataset", cols=9, remove=True, symmetry=False, noise=ZERO, frames=[2, 1, 0],
         class_names=CLASSES, groups=[dict(pedestrian=20), dict(car=18), dict(traffic_cone=21)]),
    # boxes 0-2 of frame 2: box 1 (car) inside box 0 (truck, masked out): every try of box 1 collides, its points are its own
    dict(name="D", type="NuScenesDataset", cols=9, remove=True, symmetry=False, noise=NOISY, frames=[2], boxes=(0, 3),
         class_names=["car"], groups=[dict(car=1)]),                       # sample_all returns None
]


def recompiled_with_value_is(fn):
    """fn's own source with ``is True`` / ``is False`` -> ``== True`` / ``== False`` (numba's meaning), in fn's globals."""
    tree = ast.parse(textwrap.dedent(inspect.getsource(fn)))

    class T(ast.NodeTransformer):
        def visit_Compare(self, node):
            self.generic_visit(node)
            if len(node.ops) == 1 and isinstance(node.ops[0], ast.Is) and isinstance(node.comparators[0], ast.Constant) \
                    and isinstance(node.comparators[0].value, bool):
                node.ops = [ast.Eq()]
            return node

    tree = ast.fix_missing_locations(T().visit(tree))
    tree.body[0].decorator_list = []
    ns = {}
    exec(compile(tree, inspect.getsourcefile(fn), "exec"), fn.__globals__, ns)
    return ns[fn.__name__]


def reference_function_source(path, name):
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name][0]
    ns = {"np": np}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns[name]


def import_reference():
    cgd, bno, geometry, StandIn = G.import_reference()
    for pkg in ("det3d.core.sampler", "det3d.core.evaluation", "det3d.core.input", "det3d.core.anchor"):
        if pkg not in sys.modules:
            R._pkg(pkg, os.path.join(R.REFERENCE_ROOT, *pkg.split(".")))
    prep = importlib.import_module("det3d.core.sampler.preprocess")
    prep.box_collision_test = recompiled_with_value_is(prep.box_collision_test)
    sample_ops = importlib.import_module("det3d.core.sampler.sample_ops")
    sys.modules["det3d.datasets.kitti.kitti_common"].drop_arrays_by_name = reference_function_source(
        os.path.join(R.REFERENCE_ROOT, "det3d", "datasets", "kitti", "kitti_common.py"), "drop_arrays_by_name")

    def build_dbsampler(cfg, logger=None):
        logger = logging.getLogger("build_dbsampler")
        prepors = []
        for c in cfg.db_prep_steps:
            if "filter_by_difficulty" in c:
                prepors.append(prep.DBFilterByDifficulty(c["filter_by_difficulty"], logger=logger))
            else:
                prepors.append(prep.DBFilterByMinNumPoint(c["filter_by_min_num_points"], logger=logger))
        grot = list(cfg.global_random_rotation_range_per_object) or None
        with open(cfg.db_info_path, "rb") as f:
            db_infos = pickle.load(f)
        return sample_ops.DataBaseSamplerV2(db_infos, cfg.sample_groups, prep.DataBasePreprocessor(prepors), cfg.rate, grot,
                                            logger=logger)

    R._mod("det3d.builder", build_dbsampler=build_dbsampler, build_anchor_generator=None, build_similarity_metric=None,
           build_box_coder=None)
    R._mod("det3d.core.evaluation.bbox_overlaps", bbox_overlaps=None)
    R._mod("det3d.core.input.voxel_generator", VoxelGenerator=None)
    R._mod("det3d.core.anchor.target_assigner", TargetAssigner=None)
    pp = importlib.import_module("det3d.datasets.pipelines.preprocess")
    return dict(cgd=cgd, bno=bno, geometry=geometry, StandIn=StandIn, prep=prep, sample_ops=sample_ops, pp=pp)


def make_pool(rng, tmp, nframes):
    raws, infos = {}, []
    for f in range(nframes):
        names = [f"f{f}_s{s}.bin" for s in range(4)]
        for s, nm in enumerate(names):
            raws[nm] = G.draw_points(rng, int(rng.integers(560, 680)))
            raws[nm][:8, :2] = rng.uniform(-0.99, 0.99, (8, 2))
        sweeps = [dict(lidar_path=os.path.join(tmp, names[s]), transform_matrix=None if (f, s) == (2, 1) else G.small_rigid(rng),
                       time_lag=float(0.05 * s + rng.uniform(0, 0.01))) for s in range(1, 4)]
        infos.append(dict(lidar_path=os.path.join(tmp, names[0]), sweeps=sweeps, token=f"tok{f}"))
    return raws, infos


def raw_rows(raws, f):
    """merged row -> (file, raw row) of frame f: the key file whole, then NSWEEPS - 1 sweeps without the close points."""
    where = []
    for s in range(NSWEEPS):
        nm = f"f{f}_s{s}.bin"
        a = raws[nm]
        keep = np.ones(len(a), bool) if s == 0 else ~((np.abs(a[:, 0]) < 1.0) & (np.abs(a[:, 1]) < 1.0))
        where += [(nm, r) for r in np.flatnonzero(keep)]
    return where


class Capture:
    """Wraps module attributes of the reference while one case runs; what they saw goes to ``self.out``."""

    def __init__(self, ref):
        self.ref, self.out, self._saved = ref, {}, []

    def _wrap(self, mod, name, after):
        orig = getattr(mod, name)
        self._saved.append((mod, name, orig))

        def f(*a, **k):
            r = orig(*a, **k)
            after(a, k, r)
            return r

        setattr(mod, name, f)

    def __enter__(self):
        prep, bno, o = self.ref["prep"], self.ref["bno"], self.out
        self._wrap(prep, "noise_per_box", lambda a, k, r: o.__setitem__("selected", np.array(r, dtype=np.int32)))

        def transform(a, k, r):
            masks, valid = np.asarray(a[2]), np.asarray(a[5], bool)
            m = (masks == 1) & valid[None, :]
            o["owner"] = np.where(m.any(1), m.argmax(1), -1).astype(np.int32)
            o["first_any"] = np.where((masks == 1).any(1), (masks == 1).argmax(1), -1).astype(np.int32)
            o["holders"] = m.sum(1).astype(np.int32)

        self._wrap(prep, "points_transform_", transform)
        self._wrap(prep, "noise_per_object_v3_", lambda a, k, r: o.__setitem__("boxes_noise", a[0].copy()))
        for nm, key in (("random_flip_both", "boxes_flip"), ("random_flip", "boxes_flip"), ("global_rotation", "boxes_rot"),
                        ("global_scaling_v2", "boxes_scale")):
            self._wrap(prep, nm, lambda a, k, r, key=key: o.__setitem__(key, r[0].copy()))
        self._wrap(bno, "points_in_rbbox", lambda a, k, r: o.__setitem__("drop", np.asarray(r).any(-1)))
        return self

    def __exit__(self, *a):
        for mod, name, orig in reversed(self._saved):
            setattr(mod, name, orig)


def main():
    ref = import_reference()
    prep, pp, bno, geometry = ref["prep"], ref["pp"], ref["bno"], ref["geometry"]
    rng = np.random.default_rng(20261022)
    tmp = tempfile.mkdtemp(prefix="al3d_trainprep_")
    try:
        raws, infos = make_pool(rng, tmp, 6)
        G.write_files(tmp, raws)
        for info in infos:
            info.update(gt_boxes=np.zeros((0, 9)), gt_names=np.array([], dtype="<U32"), gt_boxes_token=np.array([], dtype="<U32"),
                        gt_boxes_velocity=np.zeros((0, 3)))

        def merged(which, path):
            with open(path, "wb") as f:
                pickle.dump([infos[i] for i in which], f)
            ds = ref["StandIn"](path, tmp, [{"type": "LoadPointCloudFromFile", "dataset": "NuScenesDataset"},
                                           {"type": "LoadPointCloudAnnotations", "with_bbox": True}], True, NSWEEPS)
            with G.pinned_choice():
                return [ds.get_sensor_data(i) for i in range(len(ds))]

        all_path = os.path.join(tmp, "infos_all.pkl")
        db_info_path = os.path.join(tmp, f"infos_train_{NSWEEPS:02d}sweeps_withvelo_{SUFFIX}.pkl")
        first = merged(range(6), all_path)
        for f, (nb, ne) in NBOX.items():
            b = G.draw_boxes(rng, first[f]["lidar"]["combined"], nb, ne)
            b[:, 6:8] = rng.normal(0, 0.5, (nb, 2))                       # column 6 is noise_per_object_v3_'s "angle"
            infos[f].update(gt_boxes=b, gt_names=np.array(rng.choice(CLASSES, nb), dtype="<U32"),
                            gt_boxes_token=np.array([f"b{f}_{i}" for i in range(nb)], dtype="<U32"),
                            gt_boxes_velocity=b[:, 6:8].copy())
        # constructed: box 1 of frame 2 sits inside box 0 (every try of either collides: selected == -1 with noise)
        infos[0]["gt_boxes"][:, 3:6] *= 0.45                              # 70 boxes in 36 m x 36 m: keep most of them apart
        g2 = infos[2]["gt_boxes"]
        g2[0, 3:6], g2[0, 8], g2[0, 6] = [9.0, 9.0, 3.0], 0.3, 0.3
        g2[1, :3], g2[1, 3:6], g2[1, 8], g2[1, 6] = g2[0, :3] + [0.4, -0.3, 0.0], [1.0, 1.2, 1.5], 0.9, 0.9
        infos[2]["gt_names"][:3] = ["truck", "car", "traffic_cone"]
        # boxes 2-9: four pairs side by side, same "angle" (column 6), a 0.12 m gap or a 0.15 m overlap: a success of the
        # first moves it to where the second would go, or the second needs some tries to get free
        for k in range(4):
            a, b = g2[2 + 2 * k], g2[3 + 2 * k]
            a[:2] = [-12.0 + 8.0 * k, 11.0 - 5.0 * (k % 2)]
            a[3:6], a[6] = [1.6, 3.4, 1.6], 0.25 * (k - 1.5)
            b[:] = a
            step = a[3] + (0.12 if k < 2 else -0.15)
            b[:2] = a[:2] + step * np.array([np.cos(a[6]), -np.sin(a[6])])
            b[8] = a[8] + 0.1
        infos[2]["gt_names"][2:10] = ["car", "car", "pedestrian", "car", "truck", "truck", "car", "pedestrian"]

        def planes_of(boxes):
            corners = bno.center_to_corner_box3d(boxes[:, :3], boxes[:, 3:6], boxes[:, -1])
            n, d = geometry.surface_equ_3d_jitv2(bno.corner_to_surfaces_3d(corners)[:, :, :3, :])
            return np.concatenate([n, d[..., None]], axis=-1)

        def noise_planes(boxes):
            return planes_of(np.ascontiguousarray(boxes[:, :7]))

        total_points = sum(len(a) for a in raws.values())
        redrawn = [0]

        def redraw(rows):
            redrawn[0] += len(rows)
            for nm, r in rows:
                raws[nm][r] = G.draw_points(rng, 1)[0]
            G.write_files(tmp, raws)
            assert redrawn[0] <= 0.01 * total_points, "more than 1 % of the points had to be redrawn"

        # ---- margin of every frame's points against its own boxes (the database builder's and the owner test's planes)
        for _ in range(20):
            frames = merged(range(6), all_path)
            bad = []
            for f, res in enumerate(frames):
                boxes = res["lidar"]["annotations"]["boxes"]
                if len(boxes) == 0:
                    continue
                ok = TN.sign_margin_ok(res["lidar"]["combined"][:, :3], planes_of(boxes)).all(1)
                ok &= TN.sign_margin_ok(res["lidar"]["combined"][:, :3], noise_planes(boxes)).all(1)
                where = raw_rows(raws, f)
                bad += [where[i] for i in np.flatnonzero(~ok)]
            if not bad:
                break
            redraw(bad)
        else:
            raise SystemExit("margin: still failing after 20 rounds")

        def build_db():
            merged(DB, db_info_path)
            with G.pinned_choice():
                ref["cgd"].create_groundtruth_database("NUSC", tmp, db_info_path, nsweeps=NSWEEPS, suffix=SUFFIX)
            pkl = os.path.join(tmp, f"dbinfos_train_{NSWEEPS}sweeps_withvelo_{SUFFIX}.pkl")
            with open(pkl, "rb") as f:
                db = pickle.load(f)
            db7 = {k: [dict(e, box3d_lidar=e["box3d_lidar"][[0, 1, 2, 3, 4, 5, 8]].copy()) for e in v] for k, v in db.items()}
            pkl7 = os.path.join(tmp, "dbinfos_7col.pkl")
            with open(pkl7, "wb") as f:
                pickle.dump(db7, f)
            return db, pkl, pkl7

        def run_case(run, pre, frame_res, seed_note):
            """One call of the reference's Preprocess -> the case dict, or the list of scene rows to redraw / 'reseed'."""
            f = frame_res["f"]
            ann = frame_res["res"]["lidar"]["annotations"]
            sl = slice(*run.get("boxes", (0, None)))
            ann = {"boxes": ann["boxes"][sl], "names": ann["names"][sl]}
            boxes = ann["boxes"] if run["cols"] == 9 else np.ascontiguousarray(ann["boxes"][:, [0, 1, 2, 3, 4, 5, 8]])
            pts = frame_res["res"]["lidar"]["combined"].copy()
            work = pts.copy()                                              # the reference works in place
            res = {"type": run["type"], "mode": "train", "metadata": {"image_prefix": tmp, "num_point_features": 5},
                   "lidar": {"points": work, "combined": work, "annotations": {"boxes": boxes.copy(), "names": ann["names"].copy()}}}
            case = {"frame": f, "in_boxes": boxes.copy(), "in_names": ann["names"].copy()}
            sampled = {}
            orig_sample_all = pre.db_sampler.sample_all

            def sample_all(*a, **k):
                r = orig_sample_all(*a, **k)
                sampled["dict"] = r
                return r

            events = set()
            orig_class = pre.db_sampler.sample_class_v2

            def sample_class_v2(name, num, gt_boxes):
                """The reference's own call; only looks at the collision matrix it computed and at the batch sampler's cursor."""
                seen, orig_ct = {}, prep.box_collision_test

                def ct(a, b, *x):
                    seen["m"] = orig_ct(a, b, *x)
                    return seen["m"].copy()

                prep.box_collision_test = ct
                try:
                    ret = orig_class(name, num, gt_boxes)
                finally:
                    prep.box_collision_test = orig_ct
                if pre.db_sampler._sampler_dict[name]._idx == 0:
                    events.add("wrap")
                m, n_gt, n0, rejected = seen["m"], gt_boxes.shape[0], len(boxes), []
                np.fill_diagonal(m, False)
                for i in range(n_gt, len(m)):
                    if m[i, :n0].any():
                        events.add("hits_gt")
                    if m[i, n0:n_gt].any():
                        events.add("hits_earlier_class")
                    live = m[i].copy()
                    live[rejected] = False
                    if m[i].any() and not live.any():
                        events.add("freed_by_rejection")
                    if live.any():
                        rejected.append(i)
                return ret

            pre.db_sampler.sample_all, pre.db_sampler.sample_class_v2 = sample_all, sample_class_v2
            for g in run["groups"]:
                (gname, gmax), = g.items()
                if gmax - int(np.sum(ann["names"] == gname)) <= 0:
                    events.add("nonpositive")
            with TN.RecordRandom() as rec, Capture(ref) as cap:
                out, _ = pre(res, None)
            pre.db_sampler.sample_all, pre.db_sampler.sample_class_v2 = orig_sample_all, orig_class
            case["events"] = np.array(sorted(events) + ([] if sampled["dict"] is not None else ["none"]), dtype="<U32")
            case["digest"] = TN.state_digest()
            case["log"] = rec.log
            sd = sampled["dict"]
            case["has_sample"] = sd is not None
            if sd is not None:
                for k in ("gt_names", "difficulty", "gt_boxes", "points", "gt_masks", "group_ids"):
                    case[f"sample_{k}"] = np.asarray(sd[k])
            gt = out["lidar"]["annotations"]
            case.update(cap.out)
            case.setdefault("drop", np.zeros(len(pts), bool))
            for k in ("owner", "first_any", "holders", "selected"):
                case.setdefault(k, np.zeros(0, np.int32))
            case.update(final_boxes=gt["gt_boxes"].copy(), final_names=np.array(gt["gt_names"]), final_classes=gt["gt_classes"].copy(),
                        cloud=out["lidar"]["points"].copy())
            bv = np.array(RANGE, dtype=np.float32)[[0, 1, 3, 4]]
            case["range_mask"] = prep.filter_gt_box_outside_range(gt["gt_boxes"], bv) if len(gt["gt_boxes"]) else np.zeros(0, bool)
            # ---- margins
            ns = len(sd["points"]) if sd is not None else 0
            all_boxes = np.concatenate([boxes, sd["gt_boxes"]]) if sd is not None else boxes
            cloud_in = np.concatenate([sd["points"], pts[~case["drop"]]]) if sd is not None else pts
            scene_ok = np.ones(len(pts), bool)
            if sd is not None and run["remove"]:
                scene_ok &= TN.sign_margin_ok(pts[:, :3], planes_of(sd["gt_boxes"])).all(1)
            if len(all_boxes):
                npl = noise_planes(all_boxes)
                scene_ok &= TN.sign_margin_ok(pts[:, :3], npl).all(1)
                if ns and not TN.sign_margin_ok(sd["points"][:, :3], npl).all():
                    return "reseed"
            if not scene_ok.all():
                where = raw_rows(raws, f)
                return [where[i] for i in np.flatnonzero(~scene_ok)]
            if run["noise"] is NOISY and len(all_boxes):
                log = rec.log
                k = [i for i, (n, v) in enumerate(log) if n == "normal"][0]
                loc, rot = log[k][1], log[k + 1][1]
                mask = np.concatenate([np.array([n in run["class_names"] for n in ann["names"]], bool),
                                       np.ones(len(all_boxes) - len(boxes), bool)])
                b32 = all_boxes.astype(np.float32)
                corners = bno.box2d_to_corner_jit(b32[:, [0, 1, 3, 4, 6]])
                margins = []
                sel = TN.noise_per_box_np(corners, b32[:, :2], mask, np.cos(rot).astype(np.float32), np.sin(rot).astype(np.float32),
                                          loc, margins=margins)
                assert np.array_equal(sel, case["selected"]), "the restatement disagrees with the reference on selected"
                if min(m[3] for m in margins) <= 1e-4:
                    return "reseed"
                case["sel_no_overwrite"] = TN.noise_per_box_np(corners, b32[:, :2], mask, np.cos(rot).astype(np.float32),
                                                              np.sin(rot).astype(np.float32), loc, overwrite=False)
            assert len(case["cloud"]) == len(cloud_in)
            return case

        def covers(mine):
            """Run A must show, on its own: all four flip outcomes, a box freed by a later try, a success that matters later."""
            flips = {tuple(int(v[1]) for v in c["log"] if v[0] == "choice") for c in mine}
            return len(flips) == 4 and any((c["selected"] > 0).any() for c in mine) and \
                any(not np.array_equal(c["selected"], c["sel_no_overwrite"]) for c in mine)

        # ---- the runs: a run whose case fails a margin that no input redraw mends takes its next seed; a redrawn scene
        # point starts everything again (the database does not read the augmented frames, the runs all do)
        reseeded = 0
        db, pkl9, pkl7 = build_db()
        for attempt in range(12):
            frames = merged(TRAIN, os.path.join(tmp, "infos_train_frames.pkl"))
            cases, again = [], False
            for ri, run in enumerate(RUNS):
                cfg = R._AttrDict(mode="train", shuffle_points=True, remove_environment=False, remove_unknown_examples=False,
                                  global_scale_noise=[0.95, 1.05], global_rot_per_obj_range=[0, 0], global_trans_noise=[0.2, 0.2, 0.2],
                                  gt_drop_percentage=0.0, gt_drop_max_keep_points=15, remove_points_after_sample=run["remove"],
                                  class_names=run["class_names"], symmetry_intensity=run["symmetry"], **run["noise"],
                                  db_sampler=R._AttrDict(type="GT-AUG", enable=False, db_info_path=pkl9 if run["cols"] == 9 else pkl7,
                                                         sample_groups=run["groups"], db_prep_steps=PREP,
                                                         global_random_rotation_range_per_object=[0, 0], rate=1.0))
                for bump in range(run.get("bump", 0), 400):
                    run["bump"] = bump
                    seed = 1000 * (ri + 1) + bump
                    np.random.seed(seed)
                    with TN.RecordRandom() as rec0:
                        pre = pp.Preprocess(cfg=cfg)
                    init_log, init_digest = rec0.log, TN.state_digest()
                    mine = []
                    for ci, f in enumerate(run["frames"]):
                        r = run_case(run, pre, dict(f=f, res=frames[TRAIN.index(f)]), None)
                        if not isinstance(r, dict):
                            break
                        r.update(run=ri, seed=seed, init_log=init_log if ci == 0 else [], init_digest=init_digest)
                        mine.append(r)
                        print(f"run {run['name']} seed {seed} case {ci}: frame {f}, boxes {len(r['in_boxes'])} + "
                              f"{len(r['sample_gt_boxes']) if r['has_sample'] else 0} sampled, selected "
                              f"{np.bincount(np.minimum(r['selected'], 1) + 1, minlength=3).tolist()} "
                              f"(-1 / 0 / later), dropped {int(r['drop'].sum())}, owned {int((r['owner'] >= 0).sum())}", flush=True)
                    if isinstance(r, dict) and run["name"] == "A" and not covers(mine):
                        print(f"run A seed {seed}: not every flip outcome / noise event; next seed", flush=True)
                        continue
                    if isinstance(r, str):
                        reseeded += 1
                        print(f"run {run['name']} seed {seed} case {ci}: a margin failed that no input redraw mends; next seed", flush=True)
                        continue
                    break
                else:
                    raise SystemExit(f"run {run['name']}: no seed passes")
                if isinstance(r, list):
                    redraw(r)
                    again = True
                    print(f"run {run['name']} case {ci}: redrew {len(r)} scene points; starting again", flush=True)
                    break
                cases += mine
            if not again:
                break
        else:
            raise SystemExit("still failing after 12 attempts")
        print(f"margin: redrew {redrawn[0]} of {total_points} raw points ({100.0 * redrawn[0] / total_points:.3f} %), "
              f"{reseeded} case reseeds")

        # ---- coverage: every rule the issue lists must have happened
        nus = [c for c in cases if RUNS[c["run"]]["type"] == "NuScenesDataset"]
        flips = {tuple(int(v[1]) for v in c["log"] if v[0] == "choice") for c in nus}
        assert flips == {(0, 0), (0, 1), (1, 0), (1, 1)}, flips
        noisy = [c for c in cases if RUNS[c["run"]]["noise"] is NOISY and "selected" in c]
        assert any((c["selected"] > 0).any() for c in noisy), "no box whose first tries collide and a later one succeeds"
        assert any(not np.array_equal(c["selected"], c["sel_no_overwrite"]) for c in noisy), "no success that makes a later box collide"
        cd = [c for c in cases if RUNS[c["run"]]["name"] == "D"][0]
        assert cd["selected"][0] == -1 and cd["selected"][1] == -1 and (cd["owner"] == 1).any() and \
            (cd["first_any"][cd["owner"] == 1] == 0).all(), "box 1 must fail every try and still own its points"
        assert any((c["holders"] >= 2).any() for c in cases), "no point inside two valid boxes"
        assert any(((c["owner"] > c["first_any"]) & (c["first_any"] >= 0)).any() for c in cases), "no point whose first box is masked"
        assert any(len(c["in_boxes"]) + (len(c["sample_gt_boxes"]) if c["has_sample"] else 0) > 64 for c in cases)
        seen = set().union(*[set(c["events"].tolist()) for c in cases])
        assert seen >= {"wrap", "hits_gt", "hits_earlier_class", "freed_by_rejection", "nonpositive", "none"}, seen
        assert any(not c["has_sample"] for c in cases) and any(c["drop"].any() for c in cases)
        assert any(c["range_mask"].any() and not c["range_mask"].all() for c in cases)

        # ---- store (the third listed sweep of a frame is never opened: its name stays in the infos, its bytes are left out)
        used = {k: v for k, v in raws.items() if not k.endswith(f"_s{NSWEEPS}.bin")}
        out = {"nsweeps": np.int64(NSWEEPS), "suffix": np.array(SUFFIX), "range": np.array(RANGE), "train_frames": np.array(TRAIN),
               "db_frames": np.array(DB), "raw_names": np.array(list(used.keys())),
               "raw_off": np.cumsum([0] + [len(a) for a in used.values()]).astype(np.int64),
               "raw_data": np.concatenate(list(used.values())), "num_runs": np.int64(len(RUNS)), "num_cases": np.int64(len(cases)),
               "prep_min_points": np.array([PREP[0]["filter_by_min_num_points"][c] for c in CLASSES]), "classes": np.array(CLASSES)}
        db_dir = os.path.join(tmp, f"gt_database_{NSWEEPS}sweeps_withvelo_{SUFFIX}")
        file_names = sorted(os.listdir(db_dir))
        files = [np.fromfile(os.path.join(db_dir, n), dtype=np.float32).reshape(-1, 5) for n in file_names]
        out.update(file_names=np.array(file_names), file_off=np.cumsum([0] + [len(a) for a in files]).astype(np.int64),
                   file_data=np.concatenate(files))
        for k, v in G.flatten(db, tmp).items():
            out[f"db_{k}"] = v
        for f, info in enumerate(infos):
            out[f"f{f}_gt_boxes"], out[f"f{f}_gt_names"] = info["gt_boxes"], info["gt_names"]
            out[f"f{f}_lidar"] = np.array(os.path.basename(info["lidar_path"]))
            out[f"f{f}_sweep_files"] = np.array([os.path.basename(s["lidar_path"]) for s in info["sweeps"]])
            out[f"f{f}_time_lag"] = np.array([s["time_lag"] for s in info["sweeps"]])
            out[f"f{f}_has_xform"] = np.array([s["transform_matrix"] is not None for s in info["sweeps"]], dtype=np.uint8)
            out[f"f{f}_xform"] = np.stack([np.eye(4) if s["transform_matrix"] is None else s["transform_matrix"]
                                           for s in info["sweeps"]])
        for f, res in zip(TRAIN, frames):
            out[f"f{f}_points"] = res["lidar"]["combined"]
        for ri, run in enumerate(RUNS):
            out[f"r{ri}_name"], out[f"r{ri}_type"], out[f"r{ri}_cols"] = np.array(run["name"]), np.array(run["type"]), np.int64(run["cols"])
            out[f"r{ri}_remove"], out[f"r{ri}_symmetry"] = np.bool_(run["remove"]), np.bool_(run["symmetry"])
            out[f"r{ri}_class_names"] = np.array(run["class_names"])
            out[f"r{ri}_group_names"] = np.array([list(g.keys())[0] for g in run["groups"]])
            out[f"r{ri}_group_nums"] = np.array([list(g.values())[0] for g in run["groups"]], dtype=np.int64)
            for k, v in run["noise"].items():
                out[f"r{ri}_{k}"] = np.array(v, dtype=np.float64)
        for ci, c in enumerate(cases):
            for key in ("log", "init_log"):
                kinds, nd, dims, vals = TN.pack_log(c.pop(key))
                out[f"c{ci}_{key}_kinds"], out[f"c{ci}_{key}_nd"], out[f"c{ci}_{key}_dims"], out[f"c{ci}_{key}_vals"] = kinds, nd, dims, vals
            for k, v in c.items():
                out[f"c{ci}_{k}"] = np.asarray(v)
        path = os.path.join(ROOT, "tests", "golden", "train_preprocess.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
