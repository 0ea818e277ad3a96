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
