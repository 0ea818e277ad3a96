"""TEST INFRASTRUCTURE ONLY.  Golden for al3d.ops.rotate_iou: the reference's own KITTI evaluation geometry on seeded pairs.

Imports det3d/datasets/utils/kitti_object_eval_python/rotate_iou.py and eval.py from the reference tree through
``oracle.ref_import.install_standins()`` -- numba as identity decorators; this file adds what those two modules need on top
(``numba.float32``, ``cuda.local.array`` handing out zeroed numpy arrays), none of which carries an algorithm -- and runs
``devRotateIoUEval`` (rotate_iou.py:250-261) pair by pair as plain Python at the four criteria, with the QUERY box first as
``rotate_iou_kernel_eval`` hands it in (:294-298), then ``d3_box_overlap_kernel`` (eval.py:129-155) on the criterion-2
results at criteria -1, 0 and 1.  The pairs are 240 KITTI camera boxes ``[x, y, z, l, h, w, ry]`` in general position, each
against a perturbed copy of itself (the reference's vertex collection is unstable on coincident edges, see
tests/test_rotated_iou_golden.py; those cases have known answers and live in tests/box_iou_cases.py instead).

Writes tests/golden/box_iou_eval.npz: ``cam_boxes`` / ``cam_query [n,7]``, their BEV rows ``boxes`` / ``query [n,5]`` =
columns (0, 2, 3, 5, 6), ``ref_k`` / ``f64_k`` for criterion k - 1 (reference float32 result, float64 yardstick),
``d3_ref_k`` / ``d3_f64_k`` for k = 0, 1, 2, and ``gap [4]`` / ``gap_d3 [3]`` = max |ref - f64| per criterion.  Needs the reference tree."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def import_reference():
    import types
    from ref_import import install_standins
    install_standins()
    nb = sys.modules["numba"]
    nb.float32, nb.int32 = np.float32, np.int32
    nb.cuda.local = types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype=dtype))
    nb.cuda.shared = nb.cuda.local
    # bare packages for the path down to the two modules: det3d/datasets/__init__.py pulls in loaders this golden never uses
    from ref_import import REFERENCE_ROOT
    path = REFERENCE_ROOT
    for name in ("det3d", "det3d.datasets", "det3d.datasets.utils", "det3d.datasets.utils.kitti_object_eval_python"):
        path = os.path.join(path, name.rsplit(".", 1)[-1])
        if name not in sys.modules:
            pkg = types.ModuleType(name)
            pkg.__path__ = [path]
            sys.modules[name] = pkg
    import importlib
    rot = importlib.import_module("det3d.datasets.utils.kitti_object_eval_python.rotate_iou")
    ev = importlib.import_module("det3d.datasets.utils.kitti_object_eval_python.eval")
    return rot, ev


def main(n=240, seed=20):
    import box_iou_cases as C
    rot, ev = import_reference()
    rng = np.random.default_rng(seed)
    foot = np.asarray(C.FOOT)[rng.integers(0, len(C.FOOT), n)] * rng.uniform(0.8, 1.2, (n, 1))
    cam = np.concatenate([rng.uniform(-40, 40, (n, 1)), rng.uniform(1.0, 2.0, (n, 1)), rng.uniform(2, 70, (n, 1)), foot[:, 1:2],
                          rng.uniform(1.3, 2.2, (n, 1)), foot[:, 0:1], rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)
    qry = cam.copy()
    qry[:, [0, 2]] += rng.uniform(-0.6, 0.6, (n, 2)).astype(np.float32)
    qry[:, 1] += rng.uniform(-0.4, 0.4, n).astype(np.float32)
    qry[:, 3:6] *= rng.uniform(0.8, 1.25, (n, 3)).astype(np.float32)
    qry[:, 6] += rng.uniform(-0.5, 0.5, n).astype(np.float32)
    bev = lambda b: np.ascontiguousarray(b[:, [0, 2, 3, 5, 6]])                      # noqa: E731
    boxes, query = bev(cam), bev(qry)
    out = dict(cam_boxes=cam, cam_query=qry, boxes=boxes, query=query)
    pad = lambda b: np.stack([b[:, 0], b[:, 1], np.zeros(len(b)), b[:, 2], b[:, 3], np.zeros(len(b)), b[:, 4]], 1).astype(np.float64)      # noqa: E731
    a64, q64 = pad(boxes), pad(query)
    inter = np.array([C.inter_matrix64(a64[i:i + 1], q64[i:i + 1], "det3d")[0, 0] for i in range(n)])
    gap = []
    for crit, metric in ((-1, "iou"), (0, "over_b"), (1, "over_a"), (2, "overlap")):
        ref = np.array([rot.devRotateIoUEval(query[i], boxes[i], crit) for i in range(n)], np.float32)
        f64 = np.array([C.metric_matrix(inter[i:i + 1, None], a64[i:i + 1], q64[i:i + 1], metric, "_bev")[0, 0] for i in range(n)])
        out[f"ref_{crit + 1}"], out[f"f64_{crit + 1}"] = ref, f64
        gap.append(float(np.abs(ref - f64).max()))
    # camera rows -> (x, z | y | l, w | h | ry): the footprint lies in the x-z plane, the height interval is [y - h, y]
    c7 = lambda b: np.stack([b[:, 0], b[:, 2], b[:, 1], b[:, 3], b[:, 5], b[:, 4], b[:, 6]], 1).astype(np.float64)      # noqa: E731
    gap_d3 = []
    for crit, metric in ((-1, "iou"), (0, "over_a"), (1, "over_b")):
        ref = np.zeros(n, np.float32)
        for i in range(n):
            rinc = np.array([[out["ref_3"][i]]], np.float32)
            ev.d3_box_overlap_kernel(cam[i:i + 1], qry[i:i + 1], rinc, crit)
            ref[i] = rinc[0, 0]
        f64 = np.array([C.metric_matrix(inter[i:i + 1, None], c7(cam[i:i + 1]), c7(qry[i:i + 1]), metric, "3d_kitti")[0, 0]
                        for i in range(n)])
        out[f"d3_ref_{crit + 1}"], out[f"d3_f64_{crit + 1}"] = ref, f64
        gap_d3.append(float(np.abs(ref - f64).max()))
    out["gap"], out["gap_d3"] = np.asarray(gap), np.asarray(gap_d3)
    path = os.path.join(ROOT, "tests", "golden", "box_iou_eval.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {n} pairs, gap {gap}, gap_d3 {gap_d3}, overlapping {(inter > 0).mean():.2f}")


if __name__ == "__main__":
    main()
