#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Golden vectors for anchor target assignment -> tests/golden/assign_targets.npz.

Runs the reference's own code, unmodified (needs the reference tree; build container only): ``AnchorGeneratorRange``,
``create_target_np`` (det3d/core/anchor/target_ops.py:28-222) in ``assign_v2``'s class loop, ``TargetAssigner.assign_v2``
itself (target_assigner.py:68-142; its three arrays must equal the class loop's, flattened its way), ``NearestIouSimilarity``
(region_similarity.py:73-91) and ``GroundBox3dCoder.encode`` (box_coders.py:32-53), after AssignTarget's ``limit_period`` on
the box angle (preprocess.py:413-417).  Stand-ins: oracle/ref_import.py's (no numba: ``iou_jit`` runs as the python loop it
is, on numpy float32 scalars, so every operation is rounded to float32); ``det3d.core.anchor`` is registered here as a bare
package so its three modules import without ``det3d/core/__init__``; ``np.meshgrid`` returns a list while the anchors are
generated (numpy >= 2 returns a tuple, which ``create_anchors_3d_range`` assigns into).

``create_target_np`` is called per class so that its ``positive_gt_id`` / ``assigned_anchors_inds`` survive (``assign_v2``
drops them): ``gt_index`` is that id mapped to the row of the frame's own list.  Per task and code column the file also holds
the float64 yardstick (``second_box_encode`` on the float32 inputs cast to float64) and the reference float32 result's own
worst absolute error against it (``ref_abs_err``).

Every condition the cases exist for is asserted below on the reference's output alone."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "assign_targets.npz")


def import_reference():
    bno = R.import_box_np_ops()
    if "det3d.core.anchor" not in sys.modules:
        R._pkg("det3d.core.anchor", os.path.join(R.REFERENCE_ROOT, "det3d", "core", "anchor"))
    mods = {n: importlib.import_module(f"det3d.core.anchor.{n}") for n in ("anchor_generator", "target_ops", "target_assigner")}
    sim = importlib.import_module("det3d.core.bbox.region_similarity")
    coders = importlib.import_module("det3d.core.bbox.box_coders")
    return bno, mods, sim, coders


def cls(name, size, matched, unmatched, rotations=(0, 1.57), z=-1.0):
    return dict(class_name=name, sizes=list(size), z=z, rotations=list(rotations), matched=matched, unmatched=unmatched)


def box(x, y, w, l, r, nd, z=-1.0, h=1.5, vx=0.0, vy=0.0):
    return [x, y, z, w, l, h, r] if nd == 7 else [x, y, z, w, l, h, vx, vy, r]


def run_case(ref, name, fm, tasks, coder, frames, rng_range):
    """One case through the reference.  ``tasks``: list of lists of ``cls``; ``frames``: list of (boxes, names)."""
    bno, mods, sim_mod, coders = ref
    nd = coder["n_dim"]
    box_coder = coders.GroundBox3dCoder(linear_dim=coder["linear"], vec_encode=coder["vec"], n_dim=nd,
                                        norm_velo=coder["norm_velo"])
    sim = sim_mod.NearestIouSimilarity()
    H, W = fm
    out = {}
    gens = []
    for t in tasks:
        gens.append([mods["anchor_generator"].AnchorGeneratorRange(
            anchor_ranges=[rng_range[0], rng_range[1], c["z"], rng_range[2], rng_range[3], c["z"]], sizes=c["sizes"],
            rotations=c["rotations"], velocities=[0, 0] if nd == 9 else None, class_name=c["class_name"],
            match_threshold=c["matched"], unmatch_threshold=c["unmatched"]) for c in t])
    assigners = [mods["target_assigner"].TargetAssigner(box_coder=box_coder, anchor_generators=g,
                                                         region_similarity_calculator=sim, positive_fraction=None,
                                                         sample_size=512) for g in gens]
    orig = np.meshgrid                 # numpy >= 2 returns a tuple, which create_anchors_3d_range assigns into
    np.meshgrid = lambda *a, **k: list(orig(*a, **k))
    try:
        dicts = [a.generate_anchors_dict([1, H, W]) for a in assigners]
    finally:
        np.meshgrid = orig

    def similarity_fn(anchors, gt_boxes):
        return sim.compare(anchors[:, [0, 1, 3, 4, -1]], gt_boxes[:, [0, 1, 3, 4, -1]])

    ci = 0
    for t, d in zip(tasks, dicts):
        for c in t:
            a = d[c["class_name"]]
            assert a["anchors"].dtype == np.float32 and a["anchors"].shape[-1] == nd
            out[f"{name}.anchors.{ci}"] = a["anchors"]
            out[f"{name}.matched.{ci}"] = a["matched_thresholds"][0]
            out[f"{name}.unmatched.{ci}"] = a["unmatched_thresholds"][0]
            assert a["matched_thresholds"].dtype == np.float32
            ci += 1
    code = box_coder.code_size
    detail = []                         # per frame, task, class: the reference's dict + overlap matrix, for the assertions
    res = {k: [[] for _ in tasks] for k in ("labels", "reg_targets", "reg_weights", "gt_index", "targets64")}
    err = [np.zeros(code) for _ in tasks]
    for b, (boxes, names) in enumerate(frames):
        boxes = np.array(boxes, dtype=np.float32).reshape(-1, nd)
        names = np.array([str(n) for n in names], dtype="<U32")
        out[f"{name}.boxes.{b}"] = boxes.copy()
        out[f"{name}.names.{b}"] = names
        lim = boxes.copy()
        lim[:, -1] = bno.limit_period(lim[:, -1], offset=0.5, period=np.pi * 2)        # preprocess.py:413-417
        assert lim.dtype == np.float32
        detail.append([])
        for ti, (t, d, assigner) in enumerate(zip(tasks, dicts, assigners)):
            # the task's boxes regrouped by class, as preprocess.py:396-411 hands them to assign_v2
            order = np.concatenate([np.where(names == c["class_name"])[0] for c in t]).astype(np.int64)
            t_boxes, t_names = lim[order], names[order]
            t_classes = np.array([[c["class_name"] for c in t].index(n) + 1 for n in t_names], dtype=np.int32)
            whole = assigner.assign_v2(d, t_boxes, None, gt_classes=t_classes, gt_names=t_names)
            lab, tgt, wgt, idx, t64 = [], [], [], [], []
            detail[b].append([])
            for k, c in enumerate(t):
                a = d[c["class_name"]]
                flat = a["anchors"].reshape(-1, nd)
                num_rot = a["anchors"].shape[-2]
                rows = np.where(names == c["class_name"])[0]
                g = np.nan_to_num(lim[rows])
                r = mods["target_ops"].create_target_np(
                    flat, g, similarity_fn, box_coder.encode, prune_anchor_fn=None,
                    gt_classes=np.full(len(rows), k + 1, np.int32), matched_threshold=a["matched_thresholds"],
                    unmatched_threshold=a["unmatched_thresholds"], positive_fraction=None, rpn_batch_size=512,
                    norm_by_num_examples=False, box_code_size=code)
                assert r["bbox_targets"].dtype == np.float32 and r["labels"].dtype == np.int32
                gi = np.full(flat.shape[0], -1, np.int32)
                y = np.zeros((flat.shape[0], code), np.float64)
                fg = r["assigned_anchors_inds"]
                if len(rows):
                    gi[fg] = rows[r["positive_gt_id"]]
                    y[fg] = bno.second_box_encode(g[r["positive_gt_id"]].astype(np.float64), flat[fg].astype(np.float64),
                                                  encode_angle_to_vector=coder["vec"], smooth_dim=coder["linear"],
                                                  norm_velo=coder["norm_velo"])
                    assert y.dtype == np.float64
                    err[ti] = np.maximum(err[ti], np.abs(r["bbox_targets"].astype(np.float64) - y).max(axis=0))
                    ov = similarity_fn(flat, g)
                    assert ov.dtype == np.float32
                else:
                    ov = np.zeros((flat.shape[0], 0), np.float32)
                detail[b][ti].append(dict(r, overlaps=ov, rows=rows, gt_index=gi))
                lab.append(r["labels"].reshape(-1, num_rot))
                wgt.append(r["bbox_outside_weights"].reshape(-1, num_rot))
                idx.append(gi.reshape(-1, num_rot))
                tgt.append(r["bbox_targets"].reshape(-1, num_rot, code))
                t64.append(y.reshape(-1, num_rot, code))
            lab, wgt, idx = (np.concatenate(v, axis=-1).reshape(-1) for v in (lab, wgt, idx))
            tgt, t64 = (np.concatenate(v, axis=-2).reshape(-1, code) for v in (tgt, t64))
            assert np.array_equal(lab, whole["labels"]) and np.array_equal(wgt, whole["bbox_outside_weights"])
            assert np.array_equal(tgt.view(np.int32), whole["bbox_targets"].view(np.int32))
            for k, v in zip(("labels", "reg_targets", "reg_weights", "gt_index", "targets64"), (lab, tgt, wgt, idx, t64)):
                res[k][ti].append(v)
    for ti in range(len(tasks)):
        for k in res:
            out[f"{name}.{k}.{ti}"] = np.stack(res[k][ti])
        out[f"{name}.ref_abs_err.{ti}"] = err[ti]
    out[f"{name}.meta"] = json.dumps(dict(
        fm=[H, W], B=len(frames), range=list(rng_range), coder=coder,
        tasks=[[dict(class_name=c["class_name"], sizes=c["sizes"], z=c["z"], rotations=c["rotations"]) for c in t]
               for t in tasks]))
    return out, detail


def occurring_thresholds(ref, fm, c, coder, boxes, rng_range):
    """Two float32 overlap values that occur as row maxima of class ``c`` on ``boxes`` without being a column maximum: the
    larger becomes the matched threshold (>= at equality), the smaller the unmatched one (strict <)."""
    _, detail = run_case(ref, "probe", fm, [[c]], coder, [(boxes, [c["class_name"]] * len(boxes))], rng_range)
    ov = detail[0][0][0]["overlaps"]
    rmax = ov.max(axis=1)
    cand = sorted({float(v) for v in rmax if v > 0 and not np.any(v == ov.max(axis=0))})
    assert len(cand) >= 2, cand
    return np.float32(cand[-1]), np.float32(cand[len(cand) // 2 - 1] if len(cand) > 2 else cand[0])


def main():
    ref = import_reference()
    out, names = {}, []
    RANGE57 = (0.0, 0.0, 28.0, 20.0)                   # 5 x 7 map, spacing 4.0: centres 2, 6, ..., 26 by 2, 6, ..., 18
    c7 = dict(n_dim=7, vec=False, linear=False, norm_velo=False)
    c9 = dict(n_dim=9, vec=True, linear=False, norm_velo=False)

    # ---- edge7: ties, a duplicate, a box far outside, a small box; n_dim 7 + scalar angle; one task of one class; B = 1
    car = cls("car", [2.0, 4.5, 1.5], 0.6, 0.45)
    b7 = [box(4.0, 2.0, 2.0, 4.5, 1.57, 7),            # a: lying, midway between the anchors at x = 2 and x = 6
          box(14.0, 10.0, 2.0, 4.5, 0.0, 7),           # b: the same box twice, exactly on an anchor
          box(14.0, 10.0, 2.0, 4.5, 0.0, 7),
          box(100.0, 100.0, 2.0, 4.5, 0.0, 7),         # c: far outside the map
          box(22.0, 14.0, 0.5, 0.5, 0.0, 7),           # d: small
          box(6.0, 15.8, 2.0, 8.0, 0.0, 7)]           # f: its second-best anchor lands between the thresholds
    o, d = run_case(ref, "edge7", (5, 7), [[car]], c7, [(b7, ["car"] * len(b7))], RANGE57)
    r = d[0][0][0]
    ov, lab, gi = r["overlaps"], r["labels"], r["gt_index"]
    tie = np.where((ov[:, 0] == ov[:, 0].max()) & (ov[:, 0] > 0))[0]
    assert len(tie) >= 2 and np.all(lab[tie] == 1) and np.all(gi[tie] == 0), "a: a tie for the box's maximum, both forced"
    assert ov[tie, 0].max() < 0.6, "a: forced, not matched"
    assert np.any(gi == 1) and not np.any(gi == 2), "b: every anchor takes the first copy"
    assert ov[:, 3].max() == 0 and not np.any(gi == 3), "c: column maximum 0, nothing forced"
    small = np.where(gi == 4)[0]
    assert len(small) >= 1 and np.all(ov[small].max(axis=1) < 0.45) and np.all(lab[small] == 1), "d: re-enabled after background"
    assert {-1, 0, 1} <= set(lab.tolist()), "f: all three label values"
    out.update(o)
    names.append("edge7")

    # ---- thr9: thresholds that occur; two tasks (two classes with different thresholds, then one class); n_dim 9 + vector
    # angle; B = 3 ragged; NaN velocity; the pi/4 and 2 pi angles; an empty frame; a class without a box; an unknown name
    e1_boxes = [box(13.0, 9.0, 3.0, 5.0, 0.3, 9, vx=1.0, vy=-2.0), box(21.0, 5.0, 2.2, 4.0, 1.2, 9)]
    e1 = cls("e1", [2.0, 4.5, 1.5], 0.6, 0.45)
    m, u = occurring_thresholds(ref, (5, 7), e1, c9, e1_boxes, RANGE57)
    assert u < m
    e1 = cls("e1", [2.0, 4.5, 1.5], float(m), float(u))
    e2 = cls("e2", [1.0, 1.0, 1.0], 0.5, 0.3, z=-0.5)
    ped = cls("ped", [0.8, 0.8, 1.8], 0.6, 0.4, rotations=(0,))
    f0 = e1_boxes + [box(6.0, 6.0, 1.1, 0.9, 0.7853, 9), box(10.0, 14.0, 1.1, 0.9, 0.7855, 9, vx=float("nan")),
                     box(18.0, 14.0, 0.9, 0.7, -3.3, 9), box(22.0, 10.0, 0.7, 0.9, 3.3, 9, vy=0.5),
                     box(3.0, 17.0, 0.9, 0.9, 0.1, 9)]
    n0 = ["e1", "e1", "e2", "e2", "ped", "ped", "e2"]
    f2 = [box(9.0, 5.0, 2.0, 4.4, -0.2, 9), box(5.0, 5.0, 1.0, 1.0, 0.0, 9), box(17.0, 13.0, 2.1, 4.6, 1.5, 9)]
    n2 = ["e1", "unknown", "e1"]
    o, d = run_case(ref, "thr9", (5, 7), [[e1, e2], [ped]], c9, [(f0, n0), ([], []), (f2, n2)], RANGE57)
    r = d[0][0][0]
    rmax = r["overlaps"].max(axis=1)
    at_m, at_u = np.where(rmax == m)[0], np.where(rmax == u)[0]
    assert len(at_m) and np.all(r["labels"][at_m] == 1), "e: >= at equality is foreground"
    assert len(at_u) and np.all(r["labels"][at_u] == -1), "e: strict <: an anchor AT the unmatched threshold is ignored"
    assert {-1, 0, 1} <= set(r["labels"].tolist()), "f"
    nan_row = d[0][0][1]
    enc = np.where(nan_row["gt_index"] == 3)[0]
    assert len(enc) and np.all(o["thr9.reg_targets.0"][0].reshape(35, 4, 10)[:, 2:, 6].reshape(-1)[enc] == 0), "g: NaN -> 0"
    assert np.isnan(o["thr9.boxes.0"][3, 6])
    for row, (xd, yd) in ((2, (1.1, 0.9)), (3, (0.9, 1.1))):                       # h: 0.7853 stands, 0.7855 lies
        bv = ref[0].rbbox2d_to_near_bbox(o["thr9.boxes.0"][row:row + 1][:, [0, 1, 3, 4, -1]])[0]
        assert np.isclose(bv[2] - bv[0], xd) and np.isclose(bv[3] - bv[1], yd), "h: near-box swap at pi / 4"
    lim = ref[0].limit_period(o["thr9.boxes.0"][4:6, -1], offset=0.5, period=np.pi * 2)
    assert lim[0] > 2.9 and lim[1] < -2.9, "h: the 2 pi limit"
    assert np.all(o["thr9.labels.0"][1] == 0) and np.all(o["thr9.labels.1"][1] == 0), "i: a frame with no box"
    assert np.all(d[2][0][1]["labels"] == 0) and np.any(d[2][0][0]["labels"] == 1), "i: a class with no box beside one with"
    out.update(o)
    names.append("thr9")

    # ---- lin16: 16 x 16 map (512 anchors per class), linear_dim + norm_velo, n_dim 9 + vector angle, B = 2
    RANGE16 = (-12.8, -12.8, 12.8, 12.8)
    cl = dict(n_dim=9, vec=True, linear=True, norm_velo=True)
    truck = cls("truck", [2.5, 6.9, 2.8], 0.55, 0.4, z=-0.4)
    cone = cls("cone", [0.4, 0.4, 1.0], 0.6, 0.4, z=-1.3)
    rng = np.random.default_rng(16)
    fl = []
    for nb in (9, 5):
        bs, ns = [], []
        for i in range(nb):
            big = i % 2 == 0
            bs.append(box(*rng.uniform(-11, 11, 2), *(rng.uniform(0.8, 1.2, 2) * ([2.5, 6.9] if big else [0.4, 0.4])),
                          rng.uniform(-4, 4), 9, z=rng.uniform(-1.5, 0), h=rng.uniform(1, 3), vx=rng.normal(), vy=rng.normal()))
            ns.append("truck" if big else "cone")
        fl.append((bs, ns))
    o, d = run_case(ref, "lin16", (16, 16), [[truck, cone]], cl, fl, RANGE16)
    assert np.any(o["lin16.labels.0"] == 1) and np.any(o["lin16.labels.0"] == 2)
    out.update(o)
    names.append("lin16")

    # ---- one7: n_dim 7 + scalar angle + linear_dim; box counts 1 and 2 per class (chunk 1 + 1), B = 1
    cl7 = dict(n_dim=7, vec=False, linear=True, norm_velo=False)
    van = cls("van", [2.0, 4.5, 1.5], 0.6, 0.45)
    bike = cls("bike", [0.6, 1.8, 1.3], 0.5, 0.35, z=-1.2)
    b1 = [box(10.5, 9.0, 2.1, 4.4, 0.05, 7), box(18.2, 6.1, 0.7, 1.7, 1.5, 7), box(5.7, 13.9, 0.6, 1.9, -0.1, 7)]
    o, d = run_case(ref, "one7", (5, 7), [[van, bike]], cl7, [(b1, ["van", "bike", "bike"])], RANGE57)
    assert np.any(o["one7.labels.0"] == 1) and np.any(o["one7.labels.0"] == 2)
    out.update(o)
    names.append("one7")

    out["cases"] = json.dumps(names)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, cases {names}")
    for n in names:
        for k in sorted(out):
            if k.startswith(n + ".ref_abs_err"):
                print(k, np.array2string(out[k], precision=3))


if __name__ == "__main__":
    main()
