"""Public mirror of the reference's voxel layers (bevfusion/mmdet3d/ops/voxel/voxelize.py ``Voxelization``,
ops/voxel/scatter_points.py ``DynamicScatter`` / ``dynamic_scatter``), inference only, on the HIP voxelizers.

* ``Voxelization(max_num_points=-1)`` (or ``max_voxels=-1``) is dynamic voxelization: ``forward(points)`` returns the
  per-point coordinates ``[N, 3] int32`` as ``(x, y, z)`` (src/voxelization_cuda.cu:56-58), ``(-1, -1, -1)`` for a point
  outside the range.  With caps it runs the hard voxelizer on one frame and returns the reference's three tensors
  ``(voxels [M, P, C], coors [M, 3] (x, y, z), num_points_per_voxel [M])``.
* ``DynamicScatter(voxel_size, point_cloud_range, average_points)``: ``forward(points, coors)`` reduces the points that
  share a coordinate row (mean or max) and returns ``(voxel_feats, voxel_coors)`` in ascending lexicographic order of the
  coordinates (``at::unique_dim``); 4-column ``coors`` carry a batch index first and are processed frame by frame with
  ``batch_size = coors[-1, 0] + 1`` like the reference.
* ``dynamic_scatter(feats, coors, reduce_type)``: the function form; rows with a negative coordinate are dropped.

The reference's atomicAdd sums in arrival order; here the float32 sum runs in ascending point index, one of its legal
orders, so results are bitwise reproducible.  There is no backward pass.
"""
import torch
from torch import nn

from .. import detector_ops as D


def dynamic_scatter(feats, coors, reduce_type="max"):
    """feats [N, C] f32, coors [N, 3] int -> (voxel_feats [M, C], voxel_coors [M, 3] int32)."""
    out, ocoors, _, _ = D.dynamic_scatter_rows(feats.contiguous(), coors.contiguous(), reduce_type)
    return out, ocoors


class Voxelization(nn.Module):
    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000, deterministic=True):
        super().__init__()
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        self.max_num_points = max_num_points
        self.max_voxels = max_voxels if isinstance(max_voxels, tuple) else (max_voxels, max_voxels)
        self.deterministic = deterministic        # both voxelizers here are deterministic
        rng = torch.tensor(point_cloud_range, dtype=torch.float32)
        grid_size = torch.round((rng[3:] - rng[:3]) / torch.tensor(voxel_size, dtype=torch.float32)).long()
        self.grid_size = grid_size
        self.pcd_shape = [*grid_size[:2], 1]
        self._vox = {}

    def _voxelizer(self, device, max_voxels):
        key = (str(device), max_voxels)
        if key not in self._vox:
            cfg = dict(range=self.point_cloud_range, voxel_size=self.voxel_size,
                       max_points_in_voxel=self.max_num_points, max_voxel_num=max_voxels)
            self._vox[key] = D.build_voxelizer(cfg, 1, device)
        return self._vox[key]

    def forward(self, input):
        max_voxels = self.max_voxels[0] if self.training else self.max_voxels[1]
        points = input.contiguous()
        vox = self._voxelizer(points.device, max_voxels)
        off = torch.tensor([0, points.shape[0]], dtype=torch.int64, device=points.device)
        if isinstance(vox, D.DynamicVoxelizer):
            return vox(points, off, want_point_coords=True)["point_coords"]
        v = vox(points, off, want_voxels=True)
        return v["voxels"], v["coords"][:, [3, 2, 1]].contiguous(), v["num_points"]

    def __repr__(self):
        return (f"{self.__class__.__name__}(voxel_size={self.voxel_size}, point_cloud_range={self.point_cloud_range}, "
                f"max_num_points={self.max_num_points}, max_voxels={self.max_voxels}, "
                f"deterministic={self.deterministic})")


class DynamicScatter(nn.Module):
    def __init__(self, voxel_size, point_cloud_range, average_points: bool):
        super().__init__()
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        self.average_points = average_points

    def forward_single(self, points, coors):
        return dynamic_scatter(points.contiguous(), coors.contiguous(), "mean" if self.average_points else "max")

    def forward(self, points, coors):
        if coors.size(-1) == 3:
            return self.forward_single(points, coors)
        batch_size = int(coors[-1, 0]) + 1
        voxels, voxel_coors = [], []
        for i in range(batch_size):
            inds = torch.where(coors[:, 0] == i)
            voxel, voxel_coor = self.forward_single(points[inds], coors[inds][:, 1:])
            voxel_coors.append(nn.functional.pad(voxel_coor, (1, 0), mode="constant", value=i))
            voxels.append(voxel)
        return torch.cat(voxels, dim=0), torch.cat(voxel_coors, dim=0)

    def __repr__(self):
        return (f"{self.__class__.__name__}(voxel_size={self.voxel_size}, point_cloud_range={self.point_cloud_range}, "
                f"average_points={self.average_points})")
