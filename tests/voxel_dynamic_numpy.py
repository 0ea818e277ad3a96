"""numpy yardstick for dynamic voxelization (test infrastructure, imports nothing of the product).

Semantics (bevfusion/mmdet3d/ops/voxel/src/voxelization_cuda.cu:19-60 + src/scatter_points_cuda.cu:183-239): c = floor((p -
range_min) / voxel_size) in float32, kept iff 0 <= c < grid; voxels = the distinct kept cells in ascending lexicographic
order of the triple (``np.unique`` on the keys); reduction over all points of the voxel: the float32 sum starts at 0 and
adds one by one in ascending point index, mean = sum / float32(count), max orders floats by bit pattern (-0 < +0)."""
import numpy as np


def grid_of(pc_range, voxel_size):
    rng = np.asarray(pc_range, np.float32)
    vs = np.asarray(voxel_size, np.float32)
    return np.round((rng[3:] - rng[:3]) / vs).astype(np.int64)


def point_coords(points, pc_range, voxel_size):
    """[N,3] int32 (x, y, z), (-1, -1, -1) for a dropped point (NaN included)."""
    rng = np.asarray(pc_range, np.float32)
    vs = np.asarray(voxel_size, np.float32)
    grid = grid_of(pc_range, voxel_size)
    with np.errstate(invalid="ignore"):
        f = np.floor((points[:, :3].astype(np.float32) - rng[:3]) / vs)
        keep = np.all((f >= np.float32(0)) & (f < grid.astype(np.float32)), axis=1)
    c = np.full((len(points), 3), -1, np.int32)
    c[keep] = f[keep].astype(np.int32)
    return c


def _ord(a):
    b = a.view(np.int32)
    return b ^ ((b >> 31) & np.int32(0x7fffffff))


def reduce_rows(feats, inv, m, reduce):
    """feats [K,C] f32 of the kept points in ascending point index, inv [K] voxel row -> ([m,C] f32, counts [m] i32)."""
    C = feats.shape[1]
    counts = np.bincount(inv, minlength=m).astype(np.int32)
    if reduce == "max":
        o = np.full((m, C), np.iinfo(np.int32).min, np.int32)
        np.maximum.at(o, inv, _ord(np.ascontiguousarray(feats)))
        return (o ^ ((o >> 31) & np.int32(0x7fffffff))).view(np.float32), counts
    acc = np.zeros((m, C), np.float32)
    for i in range(len(feats)):            # sequential float32 adds, ascending point index
        acc[inv[i]] = acc[inv[i]] + feats[i]
    if reduce == "mean":
        acc = acc / counts.astype(np.float32)[:, None]
    return acc.astype(np.float32), counts


def scatter(feats, coors, reduce):
    """dynamic_scatter on given [N,3] int coordinates: rows with a negative entry dropped, voxels sorted ascending.
    -> (voxel_feats [M,C], voxel_coors [M,3] i32, point2voxel [N] i32 (-1 dropped), counts [M] i32)."""
    coors = np.asarray(coors, np.int64)
    keep = np.all(coors >= 0, axis=1)
    p2v = np.full(len(coors), -1, np.int32)
    if not keep.any():
        return (np.zeros((0, feats.shape[1]), np.float32), np.zeros((0, 3), np.int32), p2v, np.zeros((0,), np.int32))
    ext = coors[keep].max(0) + 1
    key = (coors[keep, 0] * ext[1] + coors[keep, 1]) * ext[2] + coors[keep, 2]
    uk, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    vc = np.stack([uk // (ext[1] * ext[2]), (uk // ext[2]) % ext[1], uk % ext[2]], 1).astype(np.int32)
    out, counts = reduce_rows(np.asarray(feats, np.float32)[keep], inv, len(uk), reduce)
    p2v[keep] = inv.astype(np.int32)
    return out, vc, p2v, counts


def voxelize_frame(points, pc_range, voxel_size, order="zyx", reduce="mean"):
    """One frame.  -> dict(feat [M,F], coords [M,3] i32 in ``order``, counts [M] i32, point2voxel [N] i32,
    point_coords [N,3] i32 (x, y, z))."""
    pc = point_coords(points, pc_range, voxel_size)
    tri = pc[:, ::-1] if order == "zyx" else pc
    feat, vc, p2v, counts = scatter(np.asarray(points, np.float32), tri, reduce)
    return dict(feat=feat, coords=vc, counts=counts, point2voxel=p2v, point_coords=pc)


def voxelize_batch(frames, pc_range, voxel_size, order="zyx", reduce="mean"):
    """Frames concatenated like the device voxelizer's output: coords [M,4] (b, triple), point2voxel rows into the batch."""
    feats, coords, counts, p2v, num = [], [], [], [], []
    base = 0
    F = frames[0].shape[1] if frames else 5
    for b, pts in enumerate(frames):
        r = voxelize_frame(pts, pc_range, voxel_size, order, reduce)
        m = len(r["counts"])
        feats.append(r["feat"].reshape(m, F))
        coords.append(np.concatenate([np.full((m, 1), b, np.int32), r["coords"]], 1))
        counts.append(r["counts"])
        p2v.append(np.where(r["point2voxel"] >= 0, r["point2voxel"] + base, -1).astype(np.int32))
        num.append(m)
        base += m
    return dict(feat=np.concatenate(feats), coords=np.concatenate(coords), counts=np.concatenate(counts),
                point2voxel=np.concatenate(p2v), num_voxels=np.array(num, np.int32))
