"""TEST INFRASTRUCTURE.  The numpy yardstick of the ground-truth database builder, and the golden pool on disk.

``signs`` / ``mask`` restate the sign rule of the reference's ``_points_in_convex_polygon_3d_jit`` (geometry.py:290-303)
on float32 arrays: numpy rounds every product and every sum to float32 and fuses nothing, which is what the reference's
python loop does on float32 scalars.  ``database`` restates the per-object loop of create_gt_database.py:101-152.  Both
are pinned to tests/golden/gt_database.npz (the reference's own output) by tests/test_gt_database_cpu.py, and are what the
GPU tests compare counts, rows and indices with at sizes the golden does not have."""
import os
import pickle

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_database.npz")
_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(GOLD) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def signs(points, planes):
    """``[P, R, 6]`` float32: ((x*n0 + y*n1) + z*n2) + d."""
    x, y, z = (points[:, None, None, c].astype(np.float32) for c in range(3))
    n = planes[None].astype(np.float32)
    return ((x * n[..., 0] + y * n[..., 1]) + z * n[..., 2]) + n[..., 3]


def mask(points, planes):
    """``[P, R]`` bool: inside iff !(sign >= 0) on all six planes (a NaN sign counts as inside)."""
    with np.errstate(invalid="ignore"):
        return ~(signs(points, planes) >= 0).any(-1)


def compact(points, point_off, planes, centres, box_off, num_features):
    """The yardstick of ``selector_ops.points_in_boxes``: -> rows [T, nf] f32, index [T] i64, counts [R] i32, offsets [R+1] i64."""
    rows, index, counts = [], [], []
    for b in range(len(point_off) - 1):
        p0, p1, r0, r1 = int(point_off[b]), int(point_off[b + 1]), int(box_off[b]), int(box_off[b + 1])
        m = mask(points[p0:p1], planes[r0:r1])
        for r in range(r0, r1):
            idx = np.flatnonzero(m[:, r - r0]) + p0
            g = points[idx, :num_features].copy()
            g[:, :3] -= centres[r]
            rows.append(g)
            index.append(idx)
            counts.append(len(idx))
    counts = np.array(counts, dtype=np.int32).reshape(-1)
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    nf = int(num_features)
    return (np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, nf), np.float32),
            np.concatenate(index).astype(np.int64) if index else np.zeros((0,), np.int64), counts, offsets)


def database(frames, db_stem, db_dir, used_classes=None, relative_path=True, masks=None):
    """create_gt_database.py:101-152 over ``frames = [(points [P, 5] f32, boxes [n, 9] f32, names [n], planes [n, 6, 4])]``
    -> ``(files {name: [k, 5] f32}, all_db_infos)``.  ``masks``: per frame, instead of the yardstick's own."""
    files, infos, group_counter = {}, {}, 0
    for index, (points, boxes, names, planes) in enumerate(frames):
        m = mask(points, planes) if masks is None else masks[index]
        group_dict = {}
        for i in range(len(boxes)):
            filename = f"{index}_{names[i]}_{i}.bin"
            g = points[m[:, i]]
            g[:, :3] -= boxes[i, :3]
            files[filename] = g[:, :5]
            if used_classes is None or names[i] in used_classes:
                e = {"name": names[i], "path": db_stem + "/" + filename if relative_path else os.path.join(db_dir, filename),
                     "image_idx": index, "gt_idx": i, "box3d_lidar": boxes[i], "num_points_in_gt": g.shape[0],
                     "difficulty": np.int32(0)}
                if i not in group_dict:
                    group_dict[i] = group_counter
                    group_counter += 1
                e["group_id"] = group_dict[i]
                infos.setdefault(names[i], []).append(e)
    return files, infos


KEYS = ["name", "path", "image_idx", "gt_idx", "box3d_lidar", "num_points_in_gt", "difficulty", "group_id"]


def assert_dbinfos(db, g, prefix, root=None):
    """``db`` (as unpickled) equals the golden's flattened dbinfos ``g[prefix_*]`` field by field, key and class order included."""
    assert list(db.keys()) == g[f"{prefix}_class_order"].tolist()
    rows = [e for v in db.values() for e in v]
    assert len(rows) == len(g[f"{prefix}_name"])
    for cls, v in db.items():
        assert all(e["name"] == cls for e in v)
    for k, e in enumerate(rows):
        assert list(e.keys()) == KEYS, (k, list(e.keys()))
        assert e["name"] == g[f"{prefix}_name"][k]
        want = str(g[f"{prefix}_path"][k])
        assert e["path"] == (want if root is None else want.replace("{root}", str(root))), (e["path"], want)
        for f in ("image_idx", "gt_idx", "num_points_in_gt", "group_id"):
            assert isinstance(e[f], (int, np.integer)) and int(e[f]) == int(g[f"{prefix}_{f}"][k]), (k, f, e[f])
        assert isinstance(e["difficulty"], np.int32) and int(e["difficulty"]) == int(g[f"{prefix}_difficulty"][k])
        b = e["box3d_lidar"]
        assert isinstance(b, np.ndarray) and b.dtype == np.float32 and b.shape == (9,)
        assert np.array_equal(b.view(np.int32), g[f"{prefix}_box3d_lidar"][k].view(np.int32)), k


def golden_files(g):
    return {str(n): g["file_data"][int(g["file_off"][i]):int(g["file_off"][i + 1])] for i, n in enumerate(g["file_names"])}


def assert_files(db_dir, g):
    """The directory holds exactly the golden's files with the golden's bytes."""
    want = golden_files(g)
    assert sorted(os.listdir(db_dir)) == sorted(want)
    for n, a in want.items():
        with open(os.path.join(db_dir, n), "rb") as f:
            assert f.read() == a.tobytes(), n


def golden_frames(g):
    return [(g[f"f{f}_points"], g[f"f{f}_boxes"], g[f"f{f}_gt_names"], g[f"f{f}_planes"]) for f in range(3)]


def write_golden_pool(g, root):
    """The golden's pool under ``root`` (absolute paths, which the reference opens as they are) -> info_path."""
    root = str(root)
    for i, n in enumerate(g["raw_names"]):
        g["raw_data"][int(g["raw_off"][i]):int(g["raw_off"][i + 1])].tofile(os.path.join(root, str(n)))
    infos = []
    for f in range(3):
        sweeps = [dict(lidar_path=os.path.join(root, str(n)),
                       transform_matrix=g[f"f{f}_xform"][s].copy() if g[f"f{f}_has_xform"][s] else None,
                       time_lag=float(g[f"f{f}_time_lag"][s])) for s, n in enumerate(g[f"f{f}_sweep_files"])]
        nb = len(g[f"f{f}_gt_boxes"])
        infos.append(dict(lidar_path=os.path.join(root, str(g[f"f{f}_lidar"])), sweeps=sweeps, token=f"tok{f}",
                          gt_boxes=g[f"f{f}_gt_boxes"].copy(), gt_names=g[f"f{f}_gt_names"].copy(),
                          gt_boxes_velocity=g[f"f{f}_gt_boxes"][:, 6:8].copy(),
                          gt_boxes_token=np.array([f"b{f}_{i}" for i in range(nb)], dtype="<U32")))
    info_path = os.path.join(root, f"infos_train_{int(g['nsweeps']):02d}sweeps_withvelo_{g['suffix']}.pkl")
    with open(info_path, "wb") as fh:
        pickle.dump(infos, fh)
    return info_path
