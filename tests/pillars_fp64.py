"""float64 restatement of the PointPillars pillar net and scatter (numpy only).

Follows the reference's PillarFeatureNet / PFNLayer / PointPillarsScatter (det3d/models/readers/pillar_encoder.py:17-211,
bevfusion/mmdet3d/models/backbones/pillar_encoder.py:47-240) slot by slot, with every P slot kept (no representative
row): decoration, the mask past num_points, linear -> eval BN -> ReLU, max over all P slots, concatenation with the
max, second layer, max again.  num_points is clipped to P and the mean divides by the clipped count.  ``xcol`` / ``ycol``
name the coordinate columns that index x and y: (3, 2) for this build's and det3d's (b, z, y, x), (1, 2) for BEVFusion's
(b, x, y, z).

``pfn_net`` also returns ``absum``: per output, the abs chain of the winning slot's sum (sum of |a*w| * |scale| plus
|shift|, through both layers, starting from the operands of each decoration's subtraction), the normaliser of the GPU
tests' error e = |got - ref| / absum.
"""
import numpy as np


def fold_bn(gamma, beta, mean, var, eps):
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return scale, np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * scale


def decorate(voxels, num_points, coords, vx, vy, x_offset, y_offset, with_distance, xcol=3, ycol=2, absolute=False):
    """[M,P,F] -> [M,P,F+5(+1)] float64, zero at and past num_points.  absolute=True: the abs chain of each decorated value
    instead (|x| + |mean| for the cluster offsets, |x| + |centre| for the centre offsets): the size of the f32 operands a
    subtraction rounds, not of its small result."""
    v = np.asarray(voxels, np.float64)
    M, P, F = v.shape
    n = np.clip(np.asarray(num_points, np.int64), 0, P)
    mask = (np.arange(P)[None, :] < n[:, None]).astype(np.float64)[..., None]
    v = v * mask
    mean = v[:, :, :3].sum(1, keepdims=True) / np.maximum(n, 1).astype(np.float64)[:, None, None]
    c = np.asarray(coords, np.float64)
    cx = c[:, xcol] * vx + x_offset
    cy = c[:, ycol] * vy + y_offset
    if absolute:
        a = np.abs(v)
        parts = [a, a[:, :, :3] + np.abs(mean), (a[:, :, 0] + np.abs(cx)[:, None])[..., None],
                 (a[:, :, 1] + np.abs(cy)[:, None])[..., None]]
    else:
        parts = [v, v[:, :, :3] - mean, (v[:, :, 0] - cx[:, None])[..., None], (v[:, :, 1] - cy[:, None])[..., None]]
    if with_distance:
        parts.append(np.sqrt((v[:, :, :3] ** 2).sum(-1, keepdims=True)))
    return np.concatenate(parts, -1) * mask


def pfn_net(voxels, num_points, coords, layers, vx, vy, x_offset, y_offset, with_distance, xcol=3, ycol=2):
    """layers: [(W [units, in], scale [units], shift [units]), ...] (1 or more).  Returns (out [M, C], absum [M, C])."""
    x = decorate(voxels, num_points, coords, vx, vy, x_offset, y_offset, with_distance, xcol, ycol)
    ax = decorate(voxels, num_points, coords, vx, vy, x_offset, y_offset, with_distance, xcol, ycol, absolute=True)
    for li, (w, scale, shift) in enumerate(layers):
        w = np.asarray(w, np.float64)
        y = np.einsum("mpk,uk->mpu", x, w) * scale + shift
        ay = np.einsum("mpk,uk->mpu", ax, np.abs(w)) * np.abs(scale) + np.abs(shift)
        y = np.maximum(y, 0.0)
        arg = y.argmax(1)                                        # [M, units] winning slot
        ymax = np.take_along_axis(y, arg[:, None, :], 1)[:, 0]
        amax = np.take_along_axis(ay, arg[:, None, :], 1)[:, 0]
        if li == len(layers) - 1:
            return ymax, amax
        P = x.shape[1]
        x = np.concatenate([y, np.repeat(ymax[:, None, :], P, 1)], -1)
        ax = np.concatenate([ay, np.repeat(amax[:, None, :], P, 1)], -1)
    raise ValueError("no layers")


def scatter_nhwc(rows, coords, batch, ny, nx, ycol=2, xcol=3):
    """rows [M, C] -> [batch, ny, nx, C] canvas, zero where there is no pillar."""
    rows = np.asarray(rows)
    out = np.zeros((batch, ny, nx, rows.shape[1]), rows.dtype)
    c = np.asarray(coords, np.int64)
    out[c[:, 0], c[:, ycol], c[:, xcol]] = rows
    return out


def make_case(rng, M, P, F=5, grid=(64, 64), batch=2, counts=None, scale=1.0):
    """Random pillars in the voxelizer's format: voxels [M,P,F] f32 zero past num_points, num_points [M] i32, coords
    [M,4] i32 (b, 0, y, x) unique per frame.  counts: explicit per-pillar counts, returned as given (a count above P
    exercises the clip; the slots hold P points)."""
    nx, ny = grid
    cells = rng.choice(batch * ny * nx, size=M, replace=False) if M else np.zeros(0, np.int64)
    b, rem = np.divmod(cells, ny * nx)
    y, x = np.divmod(rem, nx)
    coords = np.stack([b, np.zeros_like(b), y, x], 1).astype(np.int32)
    n = rng.integers(1, P + 1, size=M) if counts is None else np.asarray(counts)
    vox = np.zeros((M, P, F), np.float32)
    for i in range(M):
        k = min(int(n[i]), P)
        pts = rng.normal(0, 1, size=(k, F))
        pts[:, 0] = (x[i] + rng.uniform(0, 1, k)) * 0.2 - 51.2
        pts[:, 1] = (y[i] + rng.uniform(0, 1, k)) * 0.2 - 51.2
        pts[:, 2] = rng.uniform(-5, 3, k)
        vox[i, :k] = (pts * scale).astype(np.float32)
    return vox, np.asarray(n).astype(np.int32), coords


def make_layers(rng, fin, filters, bn_eps=1e-3):
    """Seeded PFN weights with non-trivial BN statistics: [(W, gamma, beta, mean, var, eps), ...] (float32 values)."""
    out, cin = [], fin
    for i, f in enumerate(filters):
        units = f if i == len(filters) - 1 else f // 2
        w = (rng.normal(0, 1, size=(units, cin)) / np.sqrt(cin)).astype(np.float32)
        g = rng.uniform(0.5, 1.5, units).astype(np.float32)
        b = rng.normal(0, 0.5, units).astype(np.float32)
        m = rng.normal(0, 0.3, units).astype(np.float32)
        v = rng.uniform(0.5, 2.0, units).astype(np.float32)
        out.append((w, g, b, m, v, bn_eps))
        cin = 2 * units
    return out
