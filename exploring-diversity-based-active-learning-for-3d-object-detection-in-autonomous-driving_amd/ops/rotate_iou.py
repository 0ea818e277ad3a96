"""det3d/datasets/utils/kitti_object_eval_python: ``rotate_iou_gpu_eval`` (rotate_iou.py:300-341) and ``bev_box_overlap`` /
``d3_box_overlap`` (eval.py:123-161) on ``selector_ops``.  numpy in, numpy out in the input dtype, as in-tree.

``rbbox_to_corners`` (rotate_iou.py:207-229) is the "det3d" convention (pinned by tests/golden/box_iou_eval.npz).  The
kernel there hands the QUERY box in first (rotate_iou.py:294-298), so criterion 0 divides by the query's area and
criterion 1 by the box's."""
import numpy as np
import torch

from .. import selector_ops as ops

_BEV = {-1: "iou_bev", 0: "over_b_bev", 1: "over_a_bev", 2: "overlap_bev"}


def _rows7(cols, device_id):
    """columns (x, y, z, s0, s1, h, r) as numpy -> ``[n, 7]`` f32 on the device"""
    rows = np.stack([np.asarray(c, np.float32) for c in cols], axis=1) if len(cols[0]) else np.zeros((0, 7), np.float32)
    return torch.from_numpy(np.ascontiguousarray(rows)).to(torch.device("cuda", device_id))


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """``boxes [N,5]``, ``query_boxes [K,5]`` = (x, y, w, l, r) -> ``[N,K]``; criterion -1 IoU, 0 inter / query area,
    1 inter / box area, anything else the intersection area."""
    boxes, query_boxes = np.asarray(boxes), np.asarray(query_boxes)
    zero = lambda b: np.zeros(len(b), np.float32)                                     # noqa: E731
    a = _rows7([boxes[:, 0], boxes[:, 1], zero(boxes), boxes[:, 2], boxes[:, 3], zero(boxes), boxes[:, 4]], device_id)
    q = query_boxes
    b = _rows7([q[:, 0], q[:, 1], zero(q), q[:, 2], q[:, 3], zero(q), q[:, 4]], device_id)
    out = ops.box_iou_matrix(a, b, metric=_BEV.get(int(criterion), "overlap_bev"), convention="det3d")
    return out.cpu().numpy().astype(boxes.dtype)


def bev_box_overlap(boxes, qboxes, criterion=-1):
    return rotate_iou_gpu_eval(boxes, qboxes, criterion)


def d3_box_overlap(boxes, qboxes, criterion=-1, device_id=0):
    """KITTI camera boxes ``[x, y, z, l, h, w, ry]``: footprint (x, z, l, w, ry), height interval [y - h, y]."""
    boxes, qboxes = np.asarray(boxes), np.asarray(qboxes)
    cam = lambda b: _rows7([b[:, 0], b[:, 2], b[:, 1], b[:, 3], b[:, 5], b[:, 4], b[:, 6]], device_id)      # noqa: E731
    metric = {-1: "iou3d_kitti", 0: "over_a3d_kitti", 1: "over_b3d_kitti"}.get(int(criterion), "overlap3d_kitti")
    out = ops.box_iou_matrix(cam(boxes), cam(qboxes), metric=metric, convention="det3d")
    if int(criterion) not in (-1, 0, 1):
        out = (out > 0).float()                            # eval.py:150-153: inc / inc
    return out.cpu().numpy().astype(boxes.dtype)
