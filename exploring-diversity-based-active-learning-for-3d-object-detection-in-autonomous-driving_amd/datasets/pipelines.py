"""Pipeline plug-ins (reference ``det3d/datasets/registry.py`` PIPELINES and
``det3d/datasets/pipelines/{loading,preprocess,formating}.py``), device-backed.

Same registry name, constructor kwargs and ``__call__(res, info) -> (res, info)`` contract as the
reference stages of the *val* pipeline; the arithmetic runs in libal3d_hip.so and the arrays they
put into ``res`` are device tensors:

* ``LoadPointCloudFromFile(dataset="NuScenesDataset")`` -- ``res["lidar"]["points" | "times" |
  "combined"]`` from the key frame + ``nsweeps-1`` sweeps (loading.py:73-126) via
  ``al3d_merge_sweeps_f32``; the sweep order comes from ``np.random.choice`` like the reference.
* ``Voxelization(cfg=dict(range, voxel_size, max_points_in_voxel, max_voxel_num))`` --
  ``res["lidar"]["voxels"] = dict(voxels, coordinates, num_points, num_voxels, shape)``
  (preprocess.py:259-304) via ``al3d_voxelize_mean_f32``; additionally ``voxel_features`` (the mean
  VFE the detector's reader would compute, voxel_encoder.py:206-211).
* ``AssignTarget(cfg=...)`` -- the constant anchors per task (preprocess.py:346-378,426-431), generated once and cached
  on the device; in train mode also ``labels`` / ``reg_targets`` / ``reg_weights`` per task (:380-479) from
  ``al3d_assign_targets_f32``.
* ``Reformat`` -- the ``example`` dict the detector reads (formating.py).
``collate_device`` is the device analogue of ``collate_kitti`` (collate.py:90-150).
"""
import numpy as np
import torch

from ..utils import Registry, build_from_cfg
from .anchors import generate_task_anchors

PIPELINES = Registry("pipeline")


def _get(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


class Compose:
    def __init__(self, transforms):
        self.transforms = [build_from_cfg(t, PIPELINES) if isinstance(t, dict) else t for t in transforms]

    def __call__(self, res, info):
        for t in self.transforms:
            res, info = t(res, info)
            if res is None:
                return None
        return res, info


@PIPELINES.register_module
class LoadPointCloudFromFile:
    def __init__(self, dataset="KittiDataset", device="cuda", root=None, **kwargs):
        self.type = dataset
        self.device = device
        self.root = root

    def __call__(self, res, info):
        res["type"] = self.type
        if self.type != "NuScenesDataset":
            raise NotImplementedError("only the NuScenesDataset branch is on the sweep path")
        from .nusc_files import load_frame_points_device
        nsweeps = res["lidar"]["nsweeps"]
        combined = load_frame_points_device(info, self.device, nsweeps=nsweeps, root=self.root, rng=np.random)
        res["lidar"]["points"] = combined[:, :4]
        res["lidar"]["times"] = combined[:, 4:5]
        res["lidar"]["combined"] = combined
        return res, info


@PIPELINES.register_module
class LoadPointCloudAnnotations:
    """loading.py:166-180.  Val mode is a pass-through (the sweep never reads annotations); with ``res["mode"] == "train"``
    the nuScenes annotations of the info go to ``res["lidar"]["annotations"]`` as float32, for ``Preprocess``."""

    def __init__(self, with_bbox=True, **kwargs):
        pass

    def __call__(self, res, info):
        if res.get("mode") == "train" and res.get("type") in ("NuScenesDataset", "LyftDataset") and "gt_boxes" in info:
            res["lidar"]["annotations"] = {
                "boxes": np.asarray(info["gt_boxes"]).astype(np.float32),
                "names": info["gt_names"],
                "tokens": info.get("gt_boxes_token"),
                "velocities": np.asarray(info["gt_boxes_velocity"]).astype(np.float32) if "gt_boxes_velocity" in info else None,
            }
        return res, info


@PIPELINES.register_module
class Preprocess:
    """preprocess.py:29-257.  Val: NuScenes points become the 5-column ``combined`` cloud; no shuffling, no filtering, no
    augmentation.  Train (:57-256): GT-AUG sampling, the per-object noise, flips, global rotation and scale, shuffle and
    ``symmetry_intensity`` through ``datasets.augment.augment_batch`` -- numpy's draws in the reference's order, the boxes
    on the host, the points in one fused launch; ``res["lidar"]["annotations"]`` becomes ``gt_boxes`` / ``gt_names`` /
    ``gt_classes``."""

    def __init__(self, cfg=None, **kwargs):
        self.mode = _get(cfg, "mode") if cfg is not None else "val"
        self.device = kwargs.get("device", "cuda")
        self._aug = None
        if self.mode == "train":
            from .augment import TrainAugmenter
            self._aug = TrainAugmenter(cfg)

    def _train(self, res):
        from .augment import augment_batch
        nusc = res["type"] == "NuScenesDataset"
        points = res["lidar"]["combined"] if nusc else res["lidar"]["points"]
        if not isinstance(points, torch.Tensor):
            points = torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32))
        points = points.to(self.device).contiguous()
        anno = res["lidar"]["annotations"]
        frame = dict(points=points, boxes=anno["boxes"], names=anno["names"], difficulty=anno.get("difficulty"),
                     image_prefix=res["metadata"]["image_prefix"], num_point_features=res["metadata"]["num_point_features"],
                     flip_both=nusc, calib=res.get("calib"))
        out = augment_batch([frame], self._aug, keep_debug=bool(res.get("keep_debug")))[0]
        res["lidar"]["points"] = out.pop("points")
        if nusc:
            res["lidar"]["combined"] = res["lidar"]["points"]            # what Voxelization reads
        res["lidar"]["annotations"] = out

    def __call__(self, res, info):
        res["mode"] = self.mode
        if self.mode == "train":
            self._train(res)
            return res, info
        if res.get("type") in ("NuScenesDataset", "LyftDataset") and res["lidar"].get("combined") is not None:
            res["lidar"]["points"] = res["lidar"]["combined"]
        return res, info


@PIPELINES.register_module
class Voxelization:
    def __init__(self, **kwargs):
        cfg = kwargs.get("cfg", None)
        self.range = _get(cfg, "range")
        self.voxel_size = _get(cfg, "voxel_size")
        self.max_points_in_voxel = _get(cfg, "max_points_in_voxel")
        self.max_voxel_num = _get(cfg, "max_voxel_num")
        self.device = kwargs.get("device", "cuda")
        self._vox = None

    def _voxelizer(self, device):
        from ..detector_ops import build_voxelizer
        if self._vox is None or self._vox.device != torch.device(device):
            cfg = dict(range=self.range, voxel_size=self.voxel_size, max_points_in_voxel=self.max_points_in_voxel,
                       max_voxel_num=self.max_voxel_num)
            self._vox = build_voxelizer(cfg, 1, device)           # dynamic when a cap is -1
        return self._vox

    def __call__(self, res, info):
        if res.get("mode", "val") == "train":                        # preprocess.py:282-288
            from .augment import filter_gt_box_outside_range
            gt_dict = res["lidar"]["annotations"]
            bv_range = np.array(self.range, dtype=np.float32)[[0, 1, 3, 4]]
            mask = filter_gt_box_outside_range(gt_dict["gt_boxes"], bv_range)
            for k in gt_dict:
                gt_dict[k] = gt_dict[k][mask]
        pts = res["lidar"].get("combined")
        if pts is None:
            pts = res["lidar"]["points"]
        if not isinstance(pts, torch.Tensor):
            pts = torch.as_tensor(np.ascontiguousarray(pts, dtype=np.float32))
        pts = pts.to(self.device).contiguous()
        vox = self._voxelizer(pts.device)
        off = torch.tensor([0, pts.shape[0]], dtype=torch.int64, device=pts.device)
        from ..detector_ops import DynamicVoxelizer
        v = vox(pts, off, want_voxels=not isinstance(vox, DynamicVoxelizer))   # no padded slots without a cap
        res["lidar"]["voxels"] = dict(
            voxels=v["voxels"],
            coordinates=v["coords"][:, 1:],                 # (z, y, x) like the reference
            num_points=v["num_points"].to(torch.int64),
            num_voxels=np.array([v["feat"].shape[0]], dtype=np.int64),
            shape=vox.grid_size,
            voxel_features=v["feat"],
        )
        return res, info


@PIPELINES.register_module
class AssignTarget:
    """preprocess.py:307-483.  Val: the constant anchors.  Train (``res["mode"] == "train"`` with ``gt_boxes`` /
    ``gt_classes`` / ``gt_names`` in ``res["lidar"]["annotations"]``): the annotations are split by task (:380-424) and
    ``labels`` / ``reg_targets`` / ``reg_weights`` per task come from one ``detector_ops.assign_targets`` launch."""

    def __init__(self, **kwargs):
        cfg = kwargs["cfg"]
        ta = _get(cfg, "target_assigner")
        self.tasks = _get(ta, "tasks")
        self.anchor_generators = _get(ta, "anchor_generators")
        self.out_size_factor = _get(cfg, "out_size_factor")
        self.device = kwargs.get("device", "cuda")
        self._cfg = cfg
        self._cache = {}
        self._plans = {}

    def _plan(self, key):
        """-> (AssignPlan, TargetAssigner per task) of a feature map; built when training first asks for it."""
        if key not in self._plans:
            from .target_assigner import build_assign_plan
            self._plans[key] = build_assign_plan(self._cfg, key, self.device)
        return self._plans[key]

    def __call__(self, res, info):
        grid = np.asarray(res["lidar"]["voxels"]["shape"])
        fm = [*(grid[:2] // self.out_size_factor), 1][::-1]          # [1, H, W]
        key = tuple(int(v) for v in fm)
        if key not in self._cache:
            self._cache[key] = [torch.as_tensor(a, dtype=torch.float32, device=self.device)
                                for a in generate_task_anchors(self.tasks, self.anchor_generators, list(key))]
        res["lidar"]["targets"] = dict(anchors=self._cache[key])
        ann = res["lidar"].get("annotations")
        if res.get("mode", "val") == "train" and isinstance(ann, dict) and all(k in ann for k in ("gt_boxes", "gt_classes", "gt_names")):
            self._train(res, key)
        return res, info

    def _train(self, res, key):
        from ..detector_ops import assign_targets
        from ..ops.box_np_ops import limit_period
        gt_dict = res["lidar"]["annotations"]
        plan, tas = self._plan(key)
        gt_classes, gt_names = np.asarray(gt_dict["gt_classes"]), np.asarray(gt_dict["gt_names"])
        gt_boxes = np.asarray(gt_dict["gt_boxes"], dtype=np.float32)
        task_boxes, task_classes, task_names, flag = [], [], [], 0
        for ta in tas:                                            # :383-411, boxes regrouped by class inside the task
            masks = [np.where(gt_classes == i + 1 + flag) for i in range(len(ta.classes))]
            task_boxes.append(np.concatenate([gt_boxes[m] for m in masks], axis=0))
            task_classes.append(np.concatenate([gt_classes[m] - flag for m in masks]))
            task_names.append(np.concatenate([gt_names[m] for m in masks]))
            flag += len(masks)
        for b in task_boxes:                                      # :413-417
            b[:, -1] = limit_period(b[:, -1], offset=0.5, period=np.pi * 2)
        gt_dict["gt_classes"], gt_dict["gt_names"], gt_dict["gt_boxes"] = task_classes, task_names, task_boxes
        # one frame, every task: the class index is the box's class position among all classes (its name inside its task)
        cls, first = [], 0
        for ta, names in zip(tas, task_names):
            cls.append(np.array([first + ta.classes.index(str(n)) if str(n) in ta.classes else -1 for n in names],
                                dtype=np.int32))
            first += len(ta.classes)
        out = assign_targets(plan, [np.concatenate(task_boxes, axis=0)], gt_class=[np.concatenate(cls)], limit_angle=False,
                             with_index=False)
        res["lidar"]["targets"].update(labels=[v[0] for v in out["labels"]], reg_targets=[v[0] for v in out["reg_targets"]],
                                       reg_weights=[v[0] for v in out["reg_weights"]])


@PIPELINES.register_module
class Reformat:
    def __init__(self, **kwargs):
        pass

    def __call__(self, res, info):
        v = res["lidar"]["voxels"]
        example = dict(metadata=res.get("metadata", {}), points=res["lidar"].get("points"),
                       voxels=v["voxels"], shape=v["shape"], num_points=v["num_points"],
                       num_voxels=v["num_voxels"], coordinates=v["coordinates"],
                       voxel_features=v.get("voxel_features"))
        if "targets" in res["lidar"]:
            example["anchors"] = res["lidar"]["targets"]["anchors"]
            for k in ("labels", "reg_targets", "reg_weights"):      # train mode (formating.py:45-57)
                if k in res["lidar"]["targets"]:
                    example[k] = res["lidar"]["targets"][k]
        return example, info


class SweepDataset:
    """Minimal dataset (val by default; ``mode="train"`` sets ``res["mode"]`` up front, nuscenes.py:156-172) (reference NuScenesDataset.get_sensor_data,
    det3d/datasets/nuscenes/nuscenes.py:139-170): ``dataset[i]`` runs the pipeline on ``infos[i]``."""

    def __init__(self, infos, pipeline, nsweeps=10, class_names=None, mode="val", root_path=None, **kwargs):
        self.mode = mode                                              # "train": the loaders fill the annotations
        self.root_path = root_path                                    # image_prefix: where the sampler finds its .bin files
        self.infos = infos
        self.nsweeps = nsweeps
        self.class_names = class_names
        self.pipeline = pipeline if isinstance(pipeline, Compose) else Compose(pipeline)

    def __len__(self):
        return len(self.infos)

    def __getitem__(self, idx):
        info = self.infos[idx]
        res = {"lidar": {"type": "lidar", "points": None, "nsweeps": self.nsweeps, "annotations": None},
               "metadata": {"image_prefix": self.root_path, "num_point_features": 5, "token": info.get("token")},
               "calib": None, "cam": {}, "mode": self.mode}
        data, _ = self.pipeline(res, info)
        return data


def collate_device(batch_list):
    """Device analogue of ``collate_kitti``: concatenate per-sample voxels and prepend the batch
    index to ``coordinates`` (``[sum M, 4]`` i32 ``(b, z, y, x)``); anchors are shared constants."""
    out = {}
    coords = []
    for b, ex in enumerate(batch_list):
        c = ex["coordinates"].to(torch.int32)
        coords.append(torch.cat([torch.full((c.shape[0], 1), b, dtype=torch.int32, device=c.device), c], dim=1))
    out["coordinates"] = torch.cat(coords, dim=0).contiguous()
    for k in ("voxels", "num_points", "voxel_features"):
        if batch_list[0].get(k) is not None:
            out[k] = torch.cat([ex[k] for ex in batch_list], dim=0)
    out["num_voxels"] = np.concatenate([np.asarray(ex["num_voxels"]) for ex in batch_list])
    out["voxel_cap"] = int(out["num_voxels"].max()) if len(out["num_voxels"]) else 0   # frames are concatenated in order
    out["shape"] = np.stack([np.asarray(ex["shape"]) for ex in batch_list])
    out["metadata"] = [ex.get("metadata") for ex in batch_list]
    if "anchors" in batch_list[0]:
        out["anchors"] = batch_list[0]["anchors"]
    return out
