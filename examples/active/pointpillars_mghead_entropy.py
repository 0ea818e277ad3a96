"""det3d's own PointPillars under the EntropySelector: PillarFeatureNet + PointPillarsScatter + RPN + MultiGroupHead in the
form det3d's PointPillars / SECOND models give the head (mg_head.py:457-459,839-842: ``loss_aux`` named direction_classifier):
0.2 m pillars on +-51.2 m, a three-block RPN (3/5/5 layers, strides 2/2/2, upsample strides 0.5/1/2) whose 128 x 128 map
feeds the six nuScenes task groups, 9-dim anchors with the SCALAR angle code (encode_angle_vector=False, code_size == n_dim),
the direction classifier (loss_aux) and rotate NMS.  Pillar and neck settings are those of
bevfusion_pointpillars_spatial_temporal_feature.py; tasks and anchors those of _cbgs_common.py."""
import os
import runpy

from al3d.models.box_coder import build_box_coder

_base_ = "bevfusion_pointpillars_spatial_temporal_feature.py"

_tasks = runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "_cbgs_common.py"))["tasks"]

box_coder = dict(type="ground_box3d_coder", n_dim=9, linear_dim=False, encode_angle_vector=False)

model = dict(
    bbox_head=dict(
        _delete_=True,                  # the base builds the embedding-only graph (bbox_head=None)
        type="MultiGroupHead", mode="3d", in_channels=sum([128, 128, 128]), norm_cfg=None, tasks=_tasks, weights=[1],
        box_coder=build_box_coder(box_coder), encode_background_as_zeros=True, use_sigmoid_score=True,
        encode_rad_error_by_sin=True,
        loss_aux=dict(type="WeightedSoftmaxClassificationLoss", name="direction_classifier", loss_weight=0.2),
        direction_offset=0.0),
)

assigner = dict(box_coder=box_coder)

selector = dict(
    type="EntropySelector",
    budget=4800,
    buffer_file="data/buffers/pointpillars_mghead_entropy.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
