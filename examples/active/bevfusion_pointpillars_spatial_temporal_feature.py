"""BEVFusion lidar-only branch with the PointPillars encoder as the embedding model of the diversity selector.  Settings
are those of the reference's bevfusion/configs/nuscenes/det/transfusion/secfpn/lidar/pointpillars.yaml,
.../secfpn/default.yaml and configs/nuscenes/default.yaml: 0.2 x 0.2 x 8 m pillars (max 20 points, 60,000 pillars at
test time), PillarFeatureNet [64, 64], a 512 x 512 canvas, a 3-block SECOND (64/128/256, strides 2/2/2, 3/5/5 layers)
and SECONDFPN (upsample strides 0.5/1/2, 3 x 128 channels), expressed on this build's det3d-shaped modules
(al3d/models/bevfusion_compat.py).  No detection head: the sweep produces the [N,384] BEV embeddings only."""
_base_ = "_cbgs_common.py"

voxel_generator = dict(
    range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0],
    voxel_size=[0.2, 0.2, 8.0],
    max_points_in_voxel=20,
    max_voxel_num=60000,            # max_voxels [train, test] = [30000, 60000]: the sweep is inference
)

_bn1d = dict(type="BN1d", eps=1e-3, momentum=0.01)
model = dict(
    _delete_=True,                  # replaces the CBGS FPNVoxelNet of the base
    type="PointPillars",
    pretrained=None,
    reader=dict(type="PillarFeatureNet", num_input_features=5, num_filters=[64, 64], with_distance=False,
                voxel_size=[0.2, 0.2, 8.0], pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], norm_cfg=_bn1d),
    backbone=dict(type="PointPillarsScatter", num_input_features=64),
    neck=dict(type="RPN", layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[64, 128, 256],
              us_layer_strides=[0.5, 1, 2], us_num_filters=[128, 128, 128], num_input_features=64,
              norm_cfg=dict(eps=1e-3, momentum=0.01)),
    bbox_head=None,
)

selector = dict(
    type="SpatialTemporalFeatureSelector",
    budget=4800,
    buffer_file="data/buffers/bevfusion_pointpillars_stf.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
