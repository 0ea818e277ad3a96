"""det3d/core/bbox/box_np_ops.py's point-in-box test on ``selector_ops`` (numpy in, numpy out).

``points_in_rbbox`` (:1102-1108) is the reference's only caller of ``points_in_convex_polygon_3d_jit`` on the data path:
the ground-truth database (create_gt_database.py:113) and the training sampler's point removal.  The planes are the
reference's own float32 calls on the host (``detector_ops.box_planes``), the sign rule runs on the device."""
import numpy as np
import torch

from .. import selector_ops as ops
from ..detector_ops import box_planes


def points_in_rbbox(points, rbbox, z_axis=2, origin=(0.5, 0.5, 0.5)):
    """``points [P, >= 3]``, ``rbbox [M, >= 7]`` float32 numpy (centre, sizes, ..., the angle LAST) -> ``[P, M]`` bool."""
    if z_axis != 2 or tuple(float(v) for v in np.ravel(origin)) != (0.5, 0.5, 0.5):
        raise NotImplementedError("points_in_rbbox: only z_axis=2 with origin=(0.5, 0.5, 0.5) is built (the lidar boxes of "
                                  f"the nuScenes path); got z_axis={z_axis!r}, origin={origin!r}")
    points, rbbox = np.asarray(points), np.asarray(rbbox)
    if points.dtype != np.float32 or rbbox.dtype != np.float32:
        raise TypeError(f"points_in_rbbox: float32 arrays expected, got {points.dtype} and {rbbox.dtype}")
    planes = torch.from_numpy(box_planes(rbbox)).cuda()
    pts = torch.from_numpy(np.ascontiguousarray(points[:, :3])).cuda()
    return ops.points_in_boxes_mask(pts, planes).cpu().numpy().astype(np.bool_)


# ---- the anchor side of target assignment (host numpy) ---------------------------------------------------------------
# Written from what the reference's functions compute (det3d/core/bbox/box_np_ops.py), under their names and arguments:
# the same float32 operations in the same order, so results equal the reference's bit for bit (tests/golden/assign_targets.npz).
def limit_period(val, offset=0.5, period=np.pi):
    """``val`` moved by whole periods into ``[-offset * period, (1 - offset) * period)`` (reference :574-575)."""
    whole = np.floor(val / period + offset)
    return val - whole * period


def center_to_minmax_2d(centers, dims, origin=0.5):
    """Centres ``[N, 2]`` and sizes ``[N, 2]`` -> ``[N, 4]`` (xmin, ymin, xmax, ymax); ``origin=0.5`` only (reference :563-571)."""
    if origin != 0.5:
        raise NotImplementedError(f"center_to_minmax_2d: only origin=0.5 is built (the near boxes of target assignment); got {origin!r}")
    half = dims / 2
    return np.concatenate((centers - half, centers + half), axis=-1)


def rbbox2d_to_near_bbox(rbboxes):
    """``[N, 5]`` (x, y, xdim, ydim, rad) -> ``[N, 4]``: the axis-aligned box of the nearer of the two orientations, upright
    (sizes as given) or lying (sizes swapped) when the angle is more than pi / 4 from the axes (reference :345-357)."""
    rbboxes = np.asarray(rbboxes)
    lying = np.abs(limit_period(rbboxes[..., 4], 0.5, np.pi)) > np.pi / 4
    sizes = rbboxes[:, 2:4].copy()
    sizes[lying] = rbboxes[lying][:, [3, 2]]
    return center_to_minmax_2d(rbboxes[:, :2], sizes)


def iou_jit(boxes, query_boxes, eps=1.0):
    """The reference's scalar loop (:957-996) as array operations: the same operations in the same order in the arrays' own
    dtype, zero where the boxes do not overlap, ``[N, K]``."""
    boxes, query_boxes = np.asarray(boxes), np.asarray(query_boxes)
    eps = boxes.dtype.type(eps)
    b, q = boxes[:, None, :], query_boxes[None, :, :]
    box_area = (q[..., 2] - q[..., 0] + eps) * (q[..., 3] - q[..., 1] + eps)
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0]) + eps
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1]) + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        ua = (b[..., 2] - b[..., 0] + eps) * (b[..., 3] - b[..., 1] + eps) + box_area - iw * ih
        ov = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), ov, boxes.dtype.type(0)).astype(boxes.dtype)


def second_box_encode(boxes, anchors, encode_angle_to_vector=False, smooth_dim=False, cylindrical=False, norm_velo=False):
    """The SECOND box code of ``boxes [N, 7 | 9]`` (x y z w l h [vx vy] r) against their ``anchors`` (reference :54-115):
    centre offsets over the anchor's footprint diagonal (z over its height), sizes as log ratios or, with ``smooth_dim``, as
    ratio - 1, velocity differences (over the diagonal with ``norm_velo``), the angle as a difference or as the difference of
    (cos, sin).  ``cylindrical`` is accepted and, as in the reference, unused.  -> ``[N, n_dim (+ 1)]``."""
    g, a = np.asarray(boxes), np.asarray(anchors)
    n_dim = a.shape[-1]
    code = np.empty((a.shape[0], n_dim + (1 if encode_angle_to_vector else 0)), dtype=np.result_type(g, a))
    footprint = np.sqrt(a[:, 4] ** 2 + a[:, 3] ** 2)
    for k, scale in ((0, footprint), (1, footprint), (2, a[:, 5])):
        code[:, k] = (g[:, k] - a[:, k]) / scale
    for k in (3, 4, 5):
        ratio = g[:, k] / a[:, k]
        code[:, k] = ratio - 1 if smooth_dim else np.log(ratio)
    if n_dim > 7:
        for k in (6, 7):
            dv = g[:, k] - a[:, k]
            code[:, k] = dv / footprint if norm_velo else dv
    if encode_angle_to_vector:
        code[:, -2] = np.cos(g[:, -1]) - np.cos(a[:, -1])
        code[:, -1] = np.sin(g[:, -1]) - np.sin(a[:, -1])
    else:
        code[:, -1] = g[:, -1] - a[:, -1]
    return code
