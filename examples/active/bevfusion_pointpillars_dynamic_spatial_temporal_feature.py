"""bevfusion_pointpillars_spatial_temporal_feature.py without point caps: dynamic voxelization (max_points_in_voxel = -1,
max_voxel_num = -1: every in-range point, every occupied pillar) and the DynamicPillarFeatureNet reader, which pools over
all points of a pillar.  The embedding of a frame is then a function of its point set and the parameters alone: no
truncation to the first 20 points of a pillar or the first 60,000 pillars in file order.  Same parameter names as the
capped config, so the same checkpoint loads.  Everything else (0.2 x 0.2 x 8 m pillars, [64, 64] filters, 512 x 512
canvas, SECOND + SECONDFPN) is that config's.  No detection head: the sweep produces the [N,384] BEV embeddings only."""
_base_ = "_cbgs_common.py"

voxel_generator = dict(
    range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0],
    voxel_size=[0.2, 0.2, 8.0],
    max_points_in_voxel=-1,         # dynamic: no cap per pillar
    max_voxel_num=-1,               # dynamic: no cap per frame
)

_bn1d = dict(type="BN1d", eps=1e-3, momentum=0.01)
model = dict(
    _delete_=True,                  # replaces the CBGS FPNVoxelNet of the base
    type="PointPillars",
    pretrained=None,
    reader=dict(type="DynamicPillarFeatureNet", num_input_features=5, num_filters=[64, 64], with_distance=False,
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
    buffer_file="data/buffers/bevfusion_pointpillars_dynamic_stf.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
