"""Drop-in mirrors of the reference's box-geometry extensions on the HIP ops of ``selector_ops``:

* ``al3d.ops.iou3d_nms``  for ``det3d.ops.iou3d_nms.iou3d_nms_utils``   (7-column boxes)
* ``al3d.ops.iou3d``      for ``mmdet3d.ops.iou3d.iou3d_utils``         ([x1, y1, x2, y2, r] rows)
* ``al3d.ops.rotate_iou`` for ``det3d.datasets.utils.kitti_object_eval_python.rotate_iou`` / ``eval`` (numpy in, numpy out)
* ``al3d.ops.points_in_rbbox`` for ``det3d.core.bbox.box_np_ops.points_in_rbbox`` (numpy in, numpy out)
"""
from . import box_np_ops, iou3d, iou3d_nms, rotate_iou  # noqa: F401
from .box_np_ops import points_in_rbbox  # noqa: F401
