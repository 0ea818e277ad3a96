"""tests/golden/train_preprocess.npz (tools/gen_golden_train_preprocess.py) unpacked for the CPU and GPU tests: the runs'
configs, the cases, and the on-disk database / pool the golden stores."""
import os
import pickle

import numpy as np

import train_preprocess_numpy as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_G = None


def golden():
    global _G
    if _G is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "train_preprocess.npz")) as z:
            _G = {k: z[k] for k in z.files}
    return _G


def num_runs():
    return int(golden()["num_runs"])


def num_cases():
    return int(golden()["num_cases"])


def case(ci):
    g, p = golden(), f"c{ci}_"
    c = {k[len(p):]: v for k, v in g.items() if k.startswith(p)}
    for key in ("log", "init_log"):
        c[key] = TN.unpack_log(c.pop(f"{key}_kinds"), c.pop(f"{key}_nd"), c.pop(f"{key}_dims"), c.pop(f"{key}_vals"))
    c["run"], c["frame"], c["seed"] = int(c["run"]), int(c["frame"]), int(c["seed"])
    c["points"] = g[f"f{c['frame']}_points"]
    return c


def cases_of(ri):
    return [ci for ci in range(num_cases()) if int(golden()[f"c{ci}_run"]) == ri]


def run(ri):
    g, p = golden(), f"r{ri}_"
    return {k[len(p):]: v for k, v in g.items() if k.startswith(p)}


def write_database(root):
    """The reference's database files and both dbinfos pickles under ``root`` -> (9-column pkl, 7-column pkl)."""
    g = golden()
    by_path = {}
    for i, name in enumerate(g["file_names"]):
        by_path[str(name)] = g["file_data"][g["file_off"][i]:g["file_off"][i + 1]]
    db = {str(k): [] for k in g["db_class_order"]}
    for i in range(len(g["db_name"])):
        rel = str(g["db_path"][i]).replace("{root}/", "")
        os.makedirs(os.path.join(root, os.path.dirname(rel)), exist_ok=True)
        by_path[os.path.basename(rel)].astype(np.float32).tofile(os.path.join(root, rel))
        db[str(g["db_name"][i])].append(dict(
            name=str(g["db_name"][i]), path=rel, image_idx=int(g["db_image_idx"][i]), gt_idx=int(g["db_gt_idx"][i]),
            box3d_lidar=g["db_box3d_lidar"][i].copy(), num_points_in_gt=int(g["db_num_points_in_gt"][i]),
            difficulty=np.int32(g["db_difficulty"][i]), group_id=int(g["db_group_id"][i])))
    p9, p7 = os.path.join(root, "dbinfos9.pkl"), os.path.join(root, "dbinfos7.pkl")
    with open(p9, "wb") as f:
        pickle.dump(db, f)
    db7 = {k: [dict(e, box3d_lidar=e["box3d_lidar"][[0, 1, 2, 3, 4, 5, 8]].copy()) for e in v] for k, v in db.items()}
    with open(p7, "wb") as f:
        pickle.dump(db7, f)
    return p9, p7


def train_cfg(ri, pkls):
    """The run's ``train_preprocessor`` dict, as tools/gen_golden_train_preprocess.py built it."""
    r, g = run(ri), golden()
    prep = [dict(filter_by_min_num_points={str(c): int(n) for c, n in zip(g["classes"], g["prep_min_points"])}),
            dict(filter_by_difficulty=[-1])]
    return dict(mode="train", shuffle_points=True, remove_environment=False, remove_unknown_examples=False,
                global_scale_noise=[0.95, 1.05], global_rot_per_obj_range=[0, 0], global_trans_noise=[0.2, 0.2, 0.2],
                gt_drop_percentage=0.0, gt_drop_max_keep_points=15, remove_points_after_sample=bool(r["remove"]),
                class_names=[str(c) for c in r["class_names"]], symmetry_intensity=bool(r["symmetry"]),
                gt_rot_noise=r["gt_rot_noise"].tolist(), gt_loc_noise=r["gt_loc_noise"].tolist(),
                global_rot_noise=r["global_rot_noise"].tolist(),
                db_sampler=dict(type="GT-AUG", enable=False, db_info_path=pkls[0] if int(r["cols"]) == 9 else pkls[1],
                                sample_groups=[{str(n): int(m)} for n, m in zip(r["group_names"], r["group_nums"])],
                                db_prep_steps=prep, global_random_rotation_range_per_object=[0, 0], rate=1.0))


def sampler_log(log):
    """The draws ``sample_all`` makes in a case: the batch samplers' reshuffles, which come before the noise draws."""
    k = [i for i, (n, _) in enumerate(log) if n == "normal"]
    return log[:k[0]] if k else [e for e in log if e[0] == "shuffle"][:-1]


def write_pool(root):
    """The pool's raw files under ``root`` -> infos (absolute paths), as the reference's loader reads them."""
    g = golden()
    for i, name in enumerate(g["raw_names"]):
        g["raw_data"][g["raw_off"][i]:g["raw_off"][i + 1]].astype(np.float32).tofile(os.path.join(root, str(name)))
    infos = []
    for f in range(6):
        sweeps = [dict(lidar_path=os.path.join(root, str(n)), transform_matrix=g[f"f{f}_xform"][s] if g[f"f{f}_has_xform"][s] else None,
                       time_lag=float(g[f"f{f}_time_lag"][s])) for s, n in enumerate(g[f"f{f}_sweep_files"])]
        b = g[f"f{f}_gt_boxes"]
        infos.append(dict(lidar_path=os.path.join(root, str(g[f"f{f}_lidar"])), sweeps=sweeps, token=f"tok{f}", gt_boxes=b,
                          gt_names=g[f"f{f}_gt_names"], gt_boxes_token=np.array([f"b{f}_{i}" for i in range(len(b))]),
                          gt_boxes_velocity=b[:, 6:8].copy()))
    return infos


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def host_inputs(c, r):
    """What the kernels of one case are fed, from the recorded draws (host numpy, the product's own box helpers)."""
    from al3d.datasets.augment import box2d_to_corner
    from al3d.detector_ops import box_planes
    boxes = c["in_boxes"]
    names = [str(n) for n in c["in_names"]]
    mask = np.array([n in [str(x) for x in r["class_names"]] for n in names], dtype=bool)
    ns, drop_planes = 0, None
    cloud = c["points"]
    if c["has_sample"]:
        boxes = np.concatenate([boxes, c["sample_gt_boxes"]])
        mask = np.concatenate([mask, c["sample_gt_masks"]])
        ns = len(c["sample_points"])
        cloud = np.concatenate([c["sample_points"], c["points"]])
        if bool(r["remove"]):
            drop_planes = box_planes(np.ascontiguousarray(c["sample_gt_boxes"], dtype=np.float32))
    log = c["log"]
    k = [i for i, (n, _) in enumerate(log) if n == "normal"][0]
    loc, rot = log[k][1], log[k + 1][1]
    rest = log[k + 3:]
    flips = [bool(v) for n, v in rest if n == "choice"]
    unis = [float(v) for n, v in rest if n == "uniform"]
    perm = [v for n, v in rest if n == "shuffle"][-1].astype(np.int64)
    b32 = np.ascontiguousarray(boxes, dtype=np.float32)
    return dict(boxes=b32, mask=mask, ns=ns, cloud=cloud, drop_planes=drop_planes, loc=loc, rot=rot,
                cos=np.cos(rot).astype(np.float32), sin=np.sin(rot).astype(np.float32),
                corners=box2d_to_corner(b32[:, [0, 1, 3, 4, 6]]), flip=(flips + [False])[:2], angle=unis[0], scale=unis[1], perm=perm,
                planes=box_planes(np.ascontiguousarray(b32[:, :7])) if len(b32) else np.zeros((0, 6, 4), np.float32))


def kept_mask(c, h):
    return np.concatenate([np.ones(h["ns"], bool), ~c["drop"].astype(bool)])
