"""Vectorised numpy restatement of anchor target assignment, written from the reference's text and independent of the
package: AssignTarget's train branch (det3d/datasets/pipelines/preprocess.py:396-479), ``assign_v2``'s class loop and
flattening (det3d/core/anchor/target_assigner.py:68-142), ``create_target_np`` (target_ops.py:28-222) with
``positive_fraction=None``, ``iou_jit(eps=0)`` on near boxes (box_np_ops.py:345-357, 957-996) and ``second_box_encode``
(:54-114).  Everything is float32 in the reference's operation order; ``encode(..., dtype=np.float64)`` is the yardstick.

Also the readers of ``tests/golden/assign_targets.npz`` and the column classes the tests compare by."""
import ctypes
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assign_targets.npz")
F32_EPS = float(np.finfo(np.float32).eps)


def limit_period(val, offset=0.5, period=np.pi):
    return val - np.floor(val / period + offset) * period


def near_bbox(rb):
    """[N, 5] (x, y, xdim, ydim, r) float32 -> [N, 4] (xmin, ymin, xmax, ymax)."""
    cond = (np.abs(limit_period(rb[:, 4], 0.5, np.pi)) > np.pi / 4)[:, None]
    c = np.where(cond, rb[:, [0, 1, 3, 2]], rb[:, :4])
    return np.concatenate([c[:, :2] - c[:, 2:] / 2, c[:, :2] + c[:, 2:] / 2], axis=-1).astype(np.float32)


def iou(boxes, query):
    """iou_jit(eps=0.0): [N, 4] x [K, 4] float32 -> [N, K] float32, the scalar loop's operations in its order."""
    b, q = boxes[:, None, :], query[None, :, :]
    zero = np.float32(0.0)
    box_area = (q[..., 2] - q[..., 0] + zero) * (q[..., 3] - q[..., 1] + zero)
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0]) + zero
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1]) + zero
    with np.errstate(divide="ignore", invalid="ignore"):
        ua = (b[..., 2] - b[..., 0] + zero) * (b[..., 3] - b[..., 1] + zero) + box_area - iw * ih
        ov = iw * ih / ua
    out = np.where((iw > 0) & (ih > 0), ov, zero)
    assert out.dtype == np.float32
    return out


def encode(boxes, anchors, vec, linear, norm_velo, dtype=np.float32):
    """second_box_encode on [N, 7 | 9] rows; ``dtype=np.float64`` evaluates the same formula on the float32 inputs."""
    g, a = boxes.astype(dtype), anchors.astype(dtype)
    nd = a.shape[1]
    xa, ya, za, wa, la, ha, ra = a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], a[:, 5], a[:, nd - 1]
    xg, yg, zg, wg, lg, hg, rg = g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4], g[:, 5], g[:, nd - 1]
    diagonal = np.sqrt(la ** 2 + wa ** 2)
    cols = [(xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / ha]
    if linear:
        lt, wt, ht = lg / la - 1, wg / wa - 1, hg / ha - 1
    else:
        lt, wt, ht = np.log(lg / la), np.log(wg / wa), np.log(hg / ha)
    cols += [wt, lt, ht]
    if nd == 9:
        vx, vy = g[:, 6] - a[:, 6], g[:, 7] - a[:, 7]
        cols += [vx / diagonal, vy / diagonal] if norm_velo else [vx, vy]
    cols += [np.cos(rg) - np.cos(ra), np.sin(rg) - np.sin(ra)] if vec else [rg - ra]
    return np.stack(cols, axis=1).astype(dtype)


def exact_columns(nd, vec, linear):
    """Columns of the code made only of + - * / sqrt (compared bit for bit), and the others (log / cos / sin)."""
    code = nd + (1 if vec else 0)
    loose = ([] if linear else [3, 4, 5]) + ([code - 2, code - 1] if vec else [])
    return [c for c in range(code) if c not in loose], loose


def create_target(anchors, anchors_bv, gt_boxes, gt_bv, matched, unmatched, label, coder):
    """create_target_np for one class.  -> labels [A] i32, targets [A, code] f32, weights [A] f32, gt_id [A] i32 (the row of
    ``gt_boxes`` an anchor is encoded against, -1 elsewhere), column maxima [G] f32."""
    A, code = anchors.shape[0], anchors.shape[1] + (1 if coder["vec"] else 0)
    labels = np.full(A, -1, np.int32)
    gt_ids = np.full(A, -1, np.int32)
    targets = np.zeros((A, code), np.float32)
    if len(gt_boxes) == 0:
        labels[:] = 0
        return labels, targets, np.zeros(A, np.float32), gt_ids, np.zeros(0, np.float32)
    ov = iou(anchors_bv, gt_bv)
    argmax = ov.argmax(axis=1)
    amax = ov[np.arange(A), argmax]
    col = ov.max(axis=0)
    col_cmp = np.where(col == 0, np.float32(-1), col)
    forced = np.where(ov == col_cmp)[0]
    labels[forced] = label
    gt_ids[forced] = argmax[forced]
    pos = amax >= np.float32(matched)
    labels[pos] = label
    gt_ids[pos] = argmax[pos]
    fg = np.where(labels > 0)[0]                       # taken before the background pass (target_ops.py:136)
    labels[amax < np.float32(unmatched)] = 0
    labels[forced] = label
    targets[fg] = encode(gt_boxes[argmax[fg]], anchors[fg], coder["vec"], coder["linear"], coder["norm_velo"])
    weights = (labels > 0).astype(np.float32)
    return labels, targets, weights, gt_ids, col


def assign_batch(tasks, coder, frames, limit_angle=True):
    """``tasks``: per task a list of dict(class_name, anchors [..., per-location anchors, nd], matched, unmatched);
    ``frames``: list of (boxes [n, nd] f32, names [n]).  -> dict of per-task lists: labels [B, A_t], reg_targets
    [B, A_t, code], reg_weights [B, A_t], gt_index [B, A_t] (rows of the frame's own list), and gt_overlap per frame."""
    out = dict(labels=[], reg_targets=[], reg_weights=[], gt_index=[], gt_overlap=[])
    prepared = []
    for boxes, names in frames:
        boxes = np.array(boxes, dtype=np.float32)
        if limit_angle and len(boxes):
            boxes[:, -1] = limit_period(boxes[:, -1], offset=0.5, period=np.pi * 2)
        boxes = np.nan_to_num(boxes)
        prepared.append((boxes, np.array([str(n) for n in names])))
        out["gt_overlap"].append(np.zeros(len(boxes), np.float32))
    for classes in tasks:
        per_frame = {k: [] for k in ("labels", "reg_targets", "reg_weights", "gt_index")}
        for b, (boxes, names) in enumerate(prepared):
            lab, tgt, wgt, idx = [], [], [], []
            for k, c in enumerate(classes):
                a = np.asarray(c["anchors"], np.float32)
                num_rot, nd = a.shape[-2], a.shape[-1]
                a = a.reshape(-1, nd)
                rows = np.where(names == c["class_name"])[0]
                g = boxes[rows]
                la, tg, wg, gi, col = create_target(a, near_bbox(a[:, [0, 1, 3, 4, -1]]), g,
                                                    near_bbox(g[:, [0, 1, 3, 4, -1]]) if len(g) else np.zeros((0, 4), np.float32),
                                                    c["matched"], c["unmatched"], k + 1, coder)
                out["gt_overlap"][b][rows] = col
                gi = np.where(gi >= 0, rows[np.maximum(gi, 0)] if len(rows) else -1, -1).astype(np.int32)
                lab.append(la.reshape(-1, num_rot))
                wgt.append(wg.reshape(-1, num_rot))
                idx.append(gi.reshape(-1, num_rot))
                tgt.append(tg.reshape(-1, num_rot, tg.shape[-1]))
            per_frame["labels"].append(np.concatenate(lab, axis=-1).reshape(-1))
            per_frame["reg_weights"].append(np.concatenate(wgt, axis=-1).reshape(-1))
            per_frame["gt_index"].append(np.concatenate(idx, axis=-1).reshape(-1))
            t = np.concatenate(tgt, axis=-2)
            per_frame["reg_targets"].append(t.reshape(-1, t.shape[-1]))
        for k, v in per_frame.items():
            out[k].append(np.stack(v) if v else None)
    return out


# ---- the golden file -------------------------------------------------------------------------------------------------
def load_golden():
    """-> list of cases: dict(name, meta, coder, tasks (with the reference's anchors), frames, and per task the reference's
    labels / reg_targets / reg_weights / gt_index [B, A_t], the float64 yardstick and ``ref_abs_err [code]``)."""
    z = np.load(GOLDEN, allow_pickle=False)
    cases = []
    for name in json.loads(str(z["cases"])):
        meta = json.loads(str(z[f"{name}.meta"]))
        tasks, ci = [], 0
        for t in meta["tasks"]:
            classes = []
            for c in t:
                classes.append(dict(c, anchors=z[f"{name}.anchors.{ci}"], matched=np.float32(z[f"{name}.matched.{ci}"]),
                                    unmatched=np.float32(z[f"{name}.unmatched.{ci}"])))
                ci += 1
            tasks.append(classes)
        frames = [(z[f"{name}.boxes.{b}"], z[f"{name}.names.{b}"]) for b in range(meta["B"])]
        case = dict(name=name, meta=meta, coder=meta["coder"], tasks=tasks, frames=frames)
        for k in ("labels", "reg_targets", "reg_weights", "gt_index", "targets64", "ref_abs_err"):
            case[k] = [z[f"{name}.{k}.{t}"] for t in range(len(tasks))]
        cases.append(case)
    return cases


def allowed_error(case, t):
    """Per column of task t's code: 0 for the exact columns; for the others the reference float32 result's own worst error
    against the float64 yardstick plus 4 float32 ulps at the column's largest intermediate magnitude (1.0 for the angle
    vector: |cos|, |sin| <= 1; the fixture's largest |log| for the size columns)."""
    coder = case["coder"]
    nd = coder["n_dim"]
    exact, loose = exact_columns(nd, coder["vec"], coder["linear"])
    tol = np.zeros(nd + (1 if coder["vec"] else 0))
    y = case["targets64"][t]
    for c in loose:
        mag = 1.0 if (coder["vec"] and c >= tol.size - 2) else max(float(np.abs(y[..., 3:6]).max()), 2.0 ** -126)
        ulp = 2.0 ** np.floor(np.log2(mag)) * F32_EPS
        tol[c] = float(case["ref_abs_err"][t][c]) + 4.0 * ulp
    return exact, loose, tol


def compare_to_golden(case, got, where=""):
    """``got``: dict of per-task lists like ``assign_batch``'s (numpy).  Integer outputs and the exact columns bit for bit,
    the log / cos / sin columns within ``allowed_error`` of the float64 yardstick.  Returns the worst error per loose column."""
    worst = {}
    for t in range(len(case["tasks"])):
        tag = f"{where}{case['name']} task {t}"
        assert np.array_equal(got["labels"][t], case["labels"][t]), f"{tag}: labels differ"
        assert np.array_equal(got["reg_weights"][t].view(np.int32), case["reg_weights"][t].view(np.int32)), f"{tag}: weights"
        if got.get("gt_index"):
            assert np.array_equal(got["gt_index"][t], case["gt_index"][t]), f"{tag}: gt_index differs"
        exact, loose, tol = allowed_error(case, t)
        g, r = np.ascontiguousarray(got["reg_targets"][t]), case["reg_targets"][t]
        assert g.shape == r.shape and g.dtype == np.float32, f"{tag}: reg_targets {g.shape} {g.dtype}"
        for c in exact:
            assert np.array_equal(g[..., c].view(np.int32), r[..., c].view(np.int32)), f"{tag}: exact column {c} differs"
        for c in loose:
            err = float(np.abs(g[..., c].astype(np.float64) - case["targets64"][t][..., c]).max()) if g.size else 0.0
            worst[(t, c)] = err
            print(f"{tag}: column {c}: error {err:.3e} against float64, allowed {tol[c]:.3e} "
                  f"(reference's own {float(case['ref_abs_err'][t][c]):.3e})")
            assert err <= tol[c], f"{tag}: column {c}: {err:.3e} > {tol[c]:.3e}"
    return worst


# ---- argument checks of the C entry (they run before any launch, so the pointers only have to be non-null) -------------
class ClassRow(ctypes.Structure):
    """al3d_assign_class_t, restated from include/al3d.h."""
    _fields_ = [("out_base", ctypes.c_int64), ("anchor_begin", ctypes.c_int), ("num_loc", ctypes.c_int),
                ("num_rot", ctypes.c_int), ("slot_offset", ctypes.c_int), ("slot_stride", ctypes.c_int),
                ("task_anchors", ctypes.c_int), ("label", ctypes.c_int), ("matched", ctypes.c_float),
                ("unmatched", ctypes.c_float)]


def _call_args(n_dim=7, A=70, R=4, B=2, gt_off=(0, 1, 4), out_rows=140, num_classes=1, classes="good", **row):
    good = dict(out_base=0, anchor_begin=0, num_loc=35, num_rot=2, slot_offset=0, slot_stride=2, task_anchors=70, label=1,
                matched=0.6, unmatched=0.45)
    good.update(row)
    tab = (ClassRow * 1)(ClassRow(**good))
    off = (ctypes.c_int * len(gt_off))(*gt_off)
    p = ctypes.c_void_p(256)
    keep = (tab, off)
    return [p, p, A, n_dim, tab if classes == "good" else None, num_classes, p, p, p, R, off, B, 0, 0, 0, p, p, p, p,
            out_rows, p], keep


def bad_argument_calls():
    """(what, arguments of al3d_assign_targets_f32, a word of the message) for every class of bad argument."""
    out = []
    for what, kw, word in (
            ("n_dim 8", dict(n_dim=8), b"n_dim"),
            ("negative A", dict(A=-1), b"count"),
            ("negative R", dict(R=-1), b"count"),
            ("negative B", dict(B=-1), b"count"),
            ("negative out_rows", dict(out_rows=-1), b"count"),
            ("no class", dict(num_classes=0), b"num_classes"),
            ("too many classes", dict(num_classes=33), b"num_classes"),
            ("null class table", dict(classes=None), b"null"),
            ("offsets that descend", dict(gt_off=(0, 3, 2)), b"ascend"),
            ("offsets past R", dict(gt_off=(0, 1, 5)), b"inside"),
            ("negative first offset", dict(gt_off=(-1, 1, 4)), b"inside"),
            ("class table overruns A", dict(A=69), b"overrun A"),
            ("class begins past A", dict(anchor_begin=1), b"overrun A"),
            ("slot overruns its task", dict(slot_offset=1), b"slot"),
            ("task size is not locations x stride", dict(task_anchors=71, out_rows=200), b"slot"),
            ("output block overruns out_rows", dict(out_rows=139), b"out_rows"),
            ("label 0", dict(label=0), b"label")):
        args, keep = _call_args(**kw)
        _KEEP.append(keep)                  # the host arrays outlive the call
        out.append((what, args + [None], word))
    return out


_KEEP = []


def bad_launch_calls():
    out = []
    for what, shape in (("0 groups", (0, 256, 64)), ("threads 96", (8, 96, 64)), ("threads 2048", (8, 2048, 64)),
                        ("chunk 0", (8, 256, 0)), ("chunk 257", (8, 256, 257))):
        args, keep = _call_args()
        _KEEP.append(keep)
        out.append((what, args + list(shape) + [None]))
    return out
