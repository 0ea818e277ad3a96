"""bevfusion/mmdet3d/ops/iou3d/iou3d_utils.py on ``selector_ops``: ``[x1, y1, x2, y2, r]`` device rows (``xywhr2xyxyr``).

The rotation is the sense of that extension's ``rotate_around_center`` (src/iou3d_kernel.cu:111-119), which is the "det3d"
convention of include/al3d.h -- the meaning csrc/center_head.hip gives such rows."""
from .. import selector_ops as ops

_ROWS = dict(convention="det3d", layout="xyxyr")


def boxes_iou_bev(boxes_a, boxes_b):
    """``[M,5]``, ``[N,5]`` -> BEV IoU ``[M,N]`` (:6-20)."""
    return ops.box_iou_matrix(boxes_a.float(), boxes_b.float(), metric="iou_bev", **_ROWS)


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """-> ``keep`` int64 on the device (:23-48)."""
    return ops.nms_boxes(boxes.float(), scores.float(), thresh, pre_max=pre_maxsize, post_max=post_max_size, **_ROWS)


def nms_normal_gpu(boxes, scores, thresh):
    """-> ``keep`` int64 on the device (:51-68)."""
    return ops.nms_boxes(boxes.float(), scores.float(), thresh, mode="normal", **_ROWS)
