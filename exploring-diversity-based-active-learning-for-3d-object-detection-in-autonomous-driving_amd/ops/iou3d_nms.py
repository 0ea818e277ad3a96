"""det3d/ops/iou3d_nms/iou3d_nms_utils.py on ``selector_ops``: the same names, signatures and return types.

Boxes are ``[n, 7]`` device rows.  ``boxes_iou_bev`` and the two NMS take ``[x, y, z, dx, dy, dz, heading]`` as the CUDA
extension does (no conversion: the "heading" convention); ``boxes_iou3d_gpu`` takes det3d's ``[x, y, z, w, l, h, r]`` -- its
``to_pcdet`` (:29-33) is folded into the "det3d" convention, the same rectangle."""
from .. import selector_ops as ops


def _seven(*boxes):
    for b in boxes:
        assert b.shape[1] == 7


def boxes_iou_bev(boxes_a, boxes_b):
    """``[N,7]``, ``[M,7]`` -> BEV IoU ``[N,M]`` (:13-27)."""
    _seven(boxes_a, boxes_b)
    return ops.box_iou_matrix(boxes_a.float(), boxes_b.float(), metric="iou_bev", convention="heading")


def boxes_iou3d_gpu(boxes_a, boxes_b):
    """``[N,7]``, ``[M,7]`` det3d boxes -> 3-D IoU ``[N,M]`` (:35-72)."""
    _seven(boxes_a, boxes_b)
    return ops.box_iou_matrix(boxes_a.float(), boxes_b.float(), metric="iou3d", convention="det3d")


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """-> ``(keep int64 on the device, None)`` (:75-90)."""
    _seven(boxes)
    return ops.nms_boxes(boxes.float(), scores.float(), thresh, pre_max=pre_maxsize, convention="heading"), None


def nms_normal_gpu(boxes, scores, thresh, **kwargs):
    """-> ``(keep int64 on the device, None)`` (:93-107)."""
    _seven(boxes)
    return ops.nms_boxes(boxes.float(), scores.float(), thresh, mode="normal", convention="heading"), None
