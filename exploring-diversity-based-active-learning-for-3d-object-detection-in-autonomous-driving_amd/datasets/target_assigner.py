"""``TargetAssigner`` under the reference's name and keywords (det3d/core/anchor/target_assigner.py), on the device.

The reference loops over a task's classes and, per class, builds the dense ``[anchors, boxes]`` overlap matrix with numba
(``create_target_np``, target_ops.py:28-222).  Here ``assign_v2`` hands one frame to ``detector_ops.assign_targets``
(csrc/assign_targets.hip); batches go to that call directly (``AssignTarget``, the loaders' ``with_targets``).  Only the
path all reference configs take is built: ``nearest_iou_similarity``, no positive / negative subsampling, no anchor mask."""
from collections import OrderedDict

import numpy as np


class NearestIouSimilarity:
    """region_similarity.py:73-91: ``iou_jit(eps=0)`` of the two lists' near boxes."""

    def compare(self, boxes1, boxes2):
        from ..ops.box_np_ops import iou_jit, rbbox2d_to_near_bbox
        return iou_jit(rbbox2d_to_near_bbox(boxes1), rbbox2d_to_near_bbox(boxes2), eps=0.0)


def build_similarity_metric(cfg):
    if isinstance(cfg, NearestIouSimilarity):
        return cfg
    kind = cfg if isinstance(cfg, str) else cfg["type"]
    if kind != "nearest_iou_similarity":
        raise NotImplementedError(f"region_similarity_calculator {kind!r}: only nearest_iou_similarity is built")
    return NearestIouSimilarity()


class TargetAssigner:
    def __init__(self, box_coder, anchor_generators, region_similarity_calculator=None, positive_fraction=None,
                 sample_size=512, device="cuda"):
        if positive_fraction is not None:
            raise NotImplementedError(f"TargetAssigner: positive_fraction={positive_fraction!r} (random positive / negative "
                                      "subsampling) is not built; the reference configs pass sample_positive_fraction=-1")
        if region_similarity_calculator is None:         # the reference's default; the one similarity that is built
            region_similarity_calculator = NearestIouSimilarity()
        if not isinstance(region_similarity_calculator, NearestIouSimilarity):
            raise NotImplementedError(f"TargetAssigner: region_similarity_calculator={region_similarity_calculator!r}: only "
                                      "nearest_iou_similarity (NearestIouSimilarity) is built")
        self._region_similarity_calculator = region_similarity_calculator
        self._box_coder = box_coder
        self._anchor_generators = anchor_generators
        self._positive_fraction = positive_fraction
        self._sample_size = sample_size
        self.device = device
        self._plans = {}

    @property
    def box_coder(self):
        return self._box_coder

    @property
    def classes(self):
        return [a.class_name for a in self._anchor_generators]

    @property
    def num_anchors_per_location(self):
        return sum(a.num_anchors_per_localization for a in self._anchor_generators)

    def _per_class(self, feature_map_size):
        """Per generator: (class name, anchors ``[D, H, W, sizes * rotations, n_dim]``, and the class's two thresholds
        repeated once per anchor in the anchors' dtype, which is how the reference hands thresholds around)."""
        for gen in self._anchor_generators:
            grid = gen.generate(feature_map_size)
            d, h, w = grid.shape[:3]
            per_class = grid.reshape(d, h, w, -1, grid.shape[-1])
            count = per_class.size // per_class.shape[-1]
            matched, unmatched = (np.full(count, v, dtype=per_class.dtype) for v in (gen.match_threshold, gen.unmatch_threshold))
            yield gen.class_name, per_class, matched, unmatched

    def generate_anchors(self, feature_map_size):
        """target_assigner.py:144-165."""
        per = list(self._per_class(feature_map_size))
        return {"anchors": np.concatenate([p[1] for p in per], axis=-2),
                "matched_thresholds": np.concatenate([p[2] for p in per], axis=0),
                "unmatched_thresholds": np.concatenate([p[3] for p in per], axis=0)}

    def generate_anchors_dict(self, feature_map_size):
        """target_assigner.py:167-187."""
        return OrderedDict((name, {"anchors": a, "matched_thresholds": m, "unmatched_thresholds": u})
                           for name, a, m, u in self._per_class(feature_map_size))

    @staticmethod
    def plan_classes(anchors_dict):
        """An ``anchors_dict`` as one task's class list for ``detector_ops.AssignPlan``."""
        out = []
        for name, d in anchors_dict.items():
            m, u = np.asarray(d["matched_thresholds"]).reshape(-1), np.asarray(d["unmatched_thresholds"]).reshape(-1)
            if m.size and (np.any(m != m[0]) or np.any(u != u[0])):
                raise NotImplementedError("TargetAssigner: per-anchor thresholds that differ inside one class are not built")
            out.append(dict(class_name=name, anchors=d["anchors"], matched=m[0] if m.size else 0.0,
                            unmatched=u[0] if u.size else 0.0))
        return out

    def _plan(self, anchors_dict):
        from ..detector_ops import AssignPlan
        key = tuple((name, id(d["anchors"])) for name, d in anchors_dict.items())
        if key not in self._plans:
            self._plans.clear()                  # one feature map at a time, like the loaders
            self._plans[key] = (AssignPlan([self.plan_classes(anchors_dict)], self._box_coder, self.device), anchors_dict)
        return self._plans[key][0]

    def assign_v2(self, anchors_dict, gt_boxes, anchors_mask=None, gt_classes=None, gt_names=None):
        """target_assigner.py:68-142 for one frame: ``labels [A_t]`` i32, ``bbox_targets [A_t, code_size]``,
        ``bbox_outside_weights [A_t]`` (numpy), anchors in (y, x, class, rotation) order.  A class's label is its position in
        the task + 1, which is what ``gt_classes`` holds in the reference's pipeline (preprocess.py:406)."""
        if anchors_mask is not None:
            raise NotImplementedError("TargetAssigner.assign_v2: anchors_mask (pos_area_threshold >= 0) is not built; the "
                                      "reference's own branch reads an undefined name (preprocess.py:437)")
        if gt_names is None:
            raise ValueError("TargetAssigner.assign_v2: gt_names is needed, one class name per row of gt_boxes (the reference "
                             "masks each class's boxes by it, target_assigner.py:82)")
        from ..detector_ops import assign_targets
        plan = self._plan(anchors_dict)
        names = [str(n) for n in gt_names]
        if len(names) != len(gt_boxes):
            raise ValueError(f"TargetAssigner.assign_v2: {len(names)} gt_names for {len(gt_boxes)} gt_boxes")
        if gt_classes is not None:
            want = np.array([plan.class_index.get(n, -1) + 1 for n in names], dtype=np.int64)
            got = np.asarray(gt_classes).astype(np.int64)
            if np.any((want > 0) & (got != want)):
                raise NotImplementedError("TargetAssigner.assign_v2: gt_classes must be each box's class position in the task "
                                          "+ 1 (labels that differ from it are not built)")
        out = assign_targets(plan, [np.ascontiguousarray(gt_boxes, dtype=np.float32)], gt_names=[names], limit_angle=False,
                             with_index=False)
        return {"labels": out["labels"][0][0].cpu().numpy(),
                "bbox_targets": out["reg_targets"][0][0].cpu().numpy(),
                "bbox_outside_weights": out["reg_weights"][0][0].cpu().numpy()}


def build_assign_plan(cfg, feature_map_size, device):
    """The config's ``assigner`` dict (``box_coder``, ``target_assigner``; what ``AssignTarget`` takes) and a feature map
    ``[1, H, W]`` -> ``(detector_ops.AssignPlan for every task, the TargetAssigner per task)``, as preprocess.py:309-340
    builds them.  Refuses what is not built and names the option."""
    from ..detector_ops import AssignPlan
    from ..models.box_coder import build_box_coder
    from .anchors import build_anchor_generator
    get = lambda c, k: c[k] if isinstance(c, dict) else getattr(c, k)  # noqa: E731
    ta = get(cfg, "target_assigner")
    if get(ta, "pos_area_threshold") >= 0:
        raise NotImplementedError("pos_area_threshold >= 0 (the anchor area mask) is not built")
    fraction = get(ta, "sample_positive_fraction")
    coder = get(cfg, "box_coder")
    coder = build_box_coder(coder) if isinstance(coder, dict) else coder
    gens = [build_anchor_generator(g) for g in get(ta, "anchor_generators")]
    sim = build_similarity_metric(get(ta, "region_similarity_calculator"))
    assigners, first = [], 0
    for t in get(ta, "tasks"):
        n = get(t, "num_class")
        assigners.append(TargetAssigner(box_coder=coder, anchor_generators=gens[first:first + n], region_similarity_calculator=sim,
                                        positive_fraction=None if fraction < 0 else fraction,
                                        sample_size=get(ta, "sample_size"), device=device))
        first += n
    fm = [int(v) for v in feature_map_size]
    plan = AssignPlan([a.plan_classes(a.generate_anchors_dict(fm)) for a in assigners], coder, device)
    return plan, assigners
