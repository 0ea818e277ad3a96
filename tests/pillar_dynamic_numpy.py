"""float64 restatement of the dynamic pillar net (csrc/pillars_dyn.hip; numpy only).

The PointPillars pillar net of tests/pillars_fp64.py over ALL points of every pillar and without padded slots: for a point
i of pillar r = point2voxel[i] (-1: skipped) the decoration is [f, xyz - mean_r, x - cx_r, y - cy_r, (|xyz|)], with mean_r
the mean of the pillar's points and (cx, cy) the centre of its cell; layer l is relu(linear * scale_l + shift_l); the first
layer's max over the pillar's points is concatenated to every point's row for the second; the output is the max over the
pillar's points (``np.maximum.at``).  No relu(shift) row of a padded slot takes part.  ``xcol`` / ``ycol`` name the
coordinate columns of x and y: (3, 2) for (b, z, y, x), (1, 2) for BEVFusion's (b, x, y, z).

``pfn_dynamic`` returns ``(ref, absum)`` like ``pillars_fp64.pfn_net``: absum is, per output, the abs chain of the winning
point's sum (sum of |a * w| * |scale| plus |shift| through both layers, starting from the operands of each decoration's
subtraction), the normaliser of the tests' error e = |got - ref| / absum.  A pillar without points gets 0 and absum 1.
"""
import numpy as np


def pfn_dynamic(points, point2voxel, coords, layers, vx, vy, x_offset, y_offset, with_distance, xcol=3, ycol=2,
                mean=None):
    """points [N,F], point2voxel [N] (row in [0, M) or -1), coords [M,4]; layers: [(W [units, in], scale, shift), ...]
    (one or two).  mean: [M, >= 3] to use in place of the pillars' own float64 mean (the kernel reads the voxelizer's).
    Returns (out [M, C], absum [M, C])."""
    pts = np.asarray(points, np.float64)
    p2v = np.asarray(point2voxel, np.int64)
    M = len(coords)
    keep = p2v >= 0
    pts, r = pts[keep], p2v[keep]
    assert (r < M).all()
    cnt = np.bincount(r, minlength=M).astype(np.float64)
    if mean is None:
        mean = np.zeros((M, 3))
        np.add.at(mean, r, pts[:, :3])
        mean = mean / np.maximum(cnt, 1.0)[:, None]
    mean = np.asarray(mean, np.float64)[:, :3]
    c = np.asarray(coords, np.float64)
    cx = c[:, xcol] * vx + x_offset
    cy = c[:, ycol] * vy + y_offset
    a = np.abs(pts)
    x = [pts, pts[:, :3] - mean[r], (pts[:, 0] - cx[r])[:, None], (pts[:, 1] - cy[r])[:, None]]
    ax = [a, a[:, :3] + np.abs(mean[r]), (a[:, 0] + np.abs(cx[r]))[:, None], (a[:, 1] + np.abs(cy[r]))[:, None]]
    if with_distance:
        d = np.sqrt((pts[:, :3] ** 2).sum(-1, keepdims=True))
        x.append(d)
        ax.append(d)
    x, ax = np.concatenate(x, -1), np.concatenate(ax, -1)
    for li, (w, scale, shift) in enumerate(layers):
        w = np.asarray(w, np.float64)
        y = np.maximum(x @ w.T * scale + shift, 0.0)
        ay = ax @ np.abs(w).T * np.abs(scale) + np.abs(shift)
        ymax = np.zeros((M, w.shape[0]))
        np.maximum.at(ymax, r, y)
        # the abs chain of a winning point (the largest among ties)
        amax = np.zeros_like(ymax)
        np.maximum.at(amax, r, np.where(y == ymax[r], ay, 0.0))
        amax[cnt == 0] = 1.0
        if li == len(layers) - 1:
            return ymax, amax
        x = np.concatenate([y, ymax[r]], -1)
        ax = np.concatenate([ay, amax[r]], -1)
    raise ValueError("no layers")


def voxelize(points, point_offsets, pc_range, voxel_size, grid):
    """Dynamic voxelization of frames concatenated in ``points``: -> (point2voxel [N] or -1, coords [M,4] (b, 0, y, x) in
    ascending (b, y, x), mean [M,F] float32: the f32 sum in ascending point index divided by (float)count)."""
    pts = np.asarray(points, np.float32)
    nx, ny = int(grid[0]), int(grid[1])
    lo = np.asarray(pc_range[:3], np.float32)
    hi = np.asarray(pc_range[3:], np.float32)
    vs = np.asarray(voxel_size, np.float32)
    b = np.searchsorted(np.asarray(point_offsets)[1:], np.arange(len(pts)), side="right")
    ij = np.floor((pts[:, :3] - lo) / vs).astype(np.int64)
    ok = ((pts[:, :3] >= lo) & (pts[:, :3] < hi)).all(1) & (ij[:, 0] >= 0) & (ij[:, 0] < nx) & (ij[:, 1] >= 0) & (ij[:, 1] < ny)
    key = (b * ny + ij[:, 1]) * nx + ij[:, 0]
    uniq, inv = np.unique(key[ok], return_inverse=True)
    p2v = np.full(len(pts), -1, np.int32)
    p2v[ok] = inv
    bb, rem = np.divmod(uniq, ny * nx)
    yy, xx = np.divmod(rem, nx)
    coords = np.stack([bb, np.zeros_like(bb), yy, xx], 1).astype(np.int32)
    mean = np.zeros((len(uniq), pts.shape[1]), np.float32)
    cnt = np.zeros(len(uniq), np.float32)
    for i in np.flatnonzero(ok):                       # ascending point index, f32 adds
        mean[p2v[i]] += pts[i]
        cnt[p2v[i]] += 1
    return p2v, coords, mean / np.maximum(cnt, 1)[:, None]
