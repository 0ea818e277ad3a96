"""GT-AUG database sampling (reference ``det3d/core/sampler/sample_ops.py`` and the sampler classes of
``det3d/core/sampler/preprocess.py:19-105``, built by ``det3d/builder.py:67-77,378-396``) under the reference's names,
constructor arguments and return dict.  Reads the ``dbinfos_train_*.pkl`` and the per-object ``.bin`` files that
``create_groundtruth_database`` writes.

Host numpy on purpose: a class has at most a few hundred candidates, and the accept loop is sequential.  Every
``np.random`` call is the reference's, in its order (the shuffles of ``BatchSampler``).  Not built, each refused by name:
group sampling (a ``sample_groups`` entry with more than one class, ``gt_group_ids``), a non-degenerate
``global_random_rotation_range_per_object`` (``noise_per_box_v2_``) and ``random_crop``.
"""
import copy
import logging
import pathlib
import pickle

import numpy as np


class BatchSampler:
    """sampler/preprocess.py:19-54."""

    def __init__(self, sampled_list, name=None, epoch=None, shuffle=True, drop_reminder=False):
        self._sampled_list = sampled_list
        self._indices = np.arange(len(sampled_list))
        if shuffle:
            np.random.shuffle(self._indices)
        self._idx = 0
        self._example_num = len(sampled_list)
        self._name = name
        self._shuffle = shuffle
        self._epoch = epoch
        self._epoch_counter = 0
        self._drop_reminder = drop_reminder

    def _sample(self, num):
        if self._idx + num >= self._example_num:
            ret = self._indices[self._idx:].copy()                         # the short tail, then a new order
            self._reset()
        else:
            ret = self._indices[self._idx:self._idx + num]
            self._idx += num
        return ret

    def _reset(self):
        if self._shuffle:
            np.random.shuffle(self._indices)
        self._idx = 0

    def sample(self, num):
        indices = self._sample(num)
        return [self._sampled_list[i] for i in indices]


class DBFilterByDifficulty:
    """sampler/preprocess.py:66-79."""

    def __init__(self, removed_difficulties, logger=None):
        self._removed_difficulties = removed_difficulties

    def __call__(self, db_infos):
        return {key: [info for info in dinfos if info["difficulty"] not in self._removed_difficulties]
                for key, dinfos in db_infos.items()}


class DBFilterByMinNumPoint:
    """sampler/preprocess.py:82-95."""

    def __init__(self, min_gt_point_dict, logger=None):
        self._min_gt_point_dict = min_gt_point_dict

    def __call__(self, db_infos):
        for name, min_num in self._min_gt_point_dict.items():
            if min_num > 0:
                db_infos[name] = [info for info in db_infos[name] if info["num_points_in_gt"] >= min_num]
        return db_infos


class DataBasePreprocessor:
    """sampler/preprocess.py:98-105."""

    def __init__(self, preprocessors):
        self._preprocessors = preprocessors

    def __call__(self, db_infos):
        for prepor in self._preprocessors:
            db_infos = prepor(db_infos)
        return db_infos


class DataBaseSamplerV2:
    """sample_ops.py:13-299 without group sampling."""

    def __init__(self, db_infos, groups, db_prepor=None, rate=1.0, global_rot_range=None, logger=None):
        logger = logger or logging.getLogger("build_dbsampler")
        for k, v in db_infos.items():
            logger.info(f"load {len(v)} {k} database infos")
        if db_prepor is not None:
            db_infos = db_prepor(db_infos)
            logger.info("After filter database:")
            for k, v in db_infos.items():
                logger.info(f"load {len(v)} {k} database infos")
        self.db_infos = db_infos
        self._rate = rate
        self._groups = groups
        self._sample_classes = []
        self._sample_max_nums = []
        if any([len(g) > 1 for g in groups]):
            raise NotImplementedError("sample_groups: a group of more than one class (group sampling) is not built")
        self._use_group_sampling = False
        self._group_db_infos = self.db_infos
        for group_info in groups:
            self._sample_classes += list(group_info.keys())
            self._sample_max_nums += list(group_info.values())
        self._sampler_dict = {k: BatchSampler(v, k) for k, v in self._group_db_infos.items()}
        if global_rot_range is not None:
            if not isinstance(global_rot_range, (list, tuple, np.ndarray)):
                global_rot_range = [-global_rot_range, global_rot_range]
            if np.abs(global_rot_range[0] - global_rot_range[1]) >= 1e-3:
                raise NotImplementedError("global_random_rotation_range_per_object: a non-degenerate range "
                                          "(noise_per_box_v2_) is not built")
        self._enable_global_rot = False
        self._global_rot_range = global_rot_range

    @property
    def use_group_sampling(self):
        return self._use_group_sampling

    def sample_all(self, root_path, gt_boxes, gt_names, num_point_features, random_crop=False, gt_group_ids=None, calib=None):
        if gt_group_ids is not None:
            raise NotImplementedError("gt_group_ids: group sampling is not built")
        if random_crop:
            raise NotImplementedError("random_crop: not built")
        sample_num_per_class = []
        for class_name, max_sample_num in zip(self._sample_classes, self._sample_max_nums):
            sampled_num = int(max_sample_num - np.sum([n == class_name for n in gt_names]))
            sample_num_per_class.append(np.round(self._rate * sampled_num).astype(np.int64))
        sampled = []
        sampled_gt_boxes = []
        avoid_coll_boxes = gt_boxes
        for class_name, sampled_num in zip(self._sample_classes, sample_num_per_class):
            if sampled_num > 0:
                sampled_cls = self.sample_class_v2(class_name, sampled_num, avoid_coll_boxes)
                sampled += sampled_cls
                if len(sampled_cls) > 0:
                    if len(sampled_cls) == 1:
                        sampled_gt_box = sampled_cls[0]["box3d_lidar"][np.newaxis, ...]
                    else:
                        sampled_gt_box = np.stack([s["box3d_lidar"] for s in sampled_cls], axis=0)
                    sampled_gt_boxes += [sampled_gt_box]
                    avoid_coll_boxes = np.concatenate([avoid_coll_boxes, sampled_gt_box], axis=0)
        if len(sampled) == 0:
            return None
        sampled_gt_boxes = np.concatenate(sampled_gt_boxes, axis=0)
        s_points_list = []
        for info in sampled:
            s_points = np.fromfile(str(pathlib.Path(root_path) / info["path"]), dtype=np.float32).reshape(-1, num_point_features)
            s_points[:, :3] += info["box3d_lidar"][:3]
            s_points_list.append(s_points)
        return {
            "gt_names": np.array([s["name"] for s in sampled]),
            "difficulty": np.array([s["difficulty"] for s in sampled]),
            "gt_boxes": sampled_gt_boxes,
            "points": np.concatenate(s_points_list, axis=0),
            "gt_masks": np.ones((len(sampled),), dtype=np.bool_),
            "group_ids": np.arange(gt_boxes.shape[0], gt_boxes.shape[0] + len(sampled)),
        }

    def sample(self, name, num):
        ret = self._sampler_dict[name].sample(num)
        return ret, np.ones((len(ret),), dtype=np.int64)

    def sample_class_v2(self, name, num, gt_boxes):
        """sample_ops.py:253-299: one collision matrix per class, then the greedy accept loop -- a rejected candidate's row
        AND column are cleared, so a later candidate that only hit it is accepted."""
        from .augment import box_collision_test, center_to_corner_box2d
        sampled = self._sampler_dict[name].sample(num)
        sampled = copy.deepcopy(sampled)
        num_gt = gt_boxes.shape[0]
        num_sampled = len(sampled)
        gt_boxes_bv = center_to_corner_box2d(gt_boxes[:, 0:2], gt_boxes[:, 3:5], gt_boxes[:, -1])
        sp_boxes = np.stack([i["box3d_lidar"] for i in sampled], axis=0)
        boxes = np.concatenate([gt_boxes, sp_boxes], axis=0).copy()
        sp_boxes_new = boxes[gt_boxes.shape[0]:]
        sp_boxes_bv = center_to_corner_box2d(sp_boxes_new[:, 0:2], sp_boxes_new[:, 3:5], sp_boxes_new[:, -1])
        total_bv = np.concatenate([gt_boxes_bv, sp_boxes_bv], axis=0)
        coll_mat = box_collision_test(total_bv, total_bv)
        diag = np.arange(total_bv.shape[0])
        coll_mat[diag, diag] = False
        valid_samples = []
        for i in range(num_gt, num_gt + num_sampled):
            if coll_mat[i].any():
                coll_mat[i] = False
                coll_mat[:, i] = False
            else:
                valid_samples.append(sampled[i - num_gt])
        return valid_samples


def build_db_preprocess(db_prep_config, logger=None):
    """builder.py:67-77."""
    cfg = db_prep_config
    if "filter_by_difficulty" in cfg:
        return DBFilterByDifficulty(cfg["filter_by_difficulty"], logger=logger)
    if "filter_by_min_num_points" in cfg:
        return DBFilterByMinNumPoint(cfg["filter_by_min_num_points"], logger=logger)
    raise ValueError("unknown database prep type")


def build_dbsampler(cfg, logger=None):
    """builder.py:378-396 (``enable`` is never read there either)."""
    get = cfg.get if hasattr(cfg, "get") else (lambda k, d=None: getattr(cfg, k, d))
    db_prepor = DataBasePreprocessor([build_db_preprocess(c, logger=logger) for c in get("db_prep_steps")])
    grot_range = list(get("global_random_rotation_range_per_object"))
    if len(grot_range) == 0:
        grot_range = None
    with open(get("db_info_path"), "rb") as f:
        db_infos = pickle.load(f)
    return DataBaseSamplerV2(db_infos, get("sample_groups"), db_prepor, get("rate"), grot_range, logger=logger)
