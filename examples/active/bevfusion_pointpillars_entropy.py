"""BEVFusion lidar-only detector with the PointPillars encoder (PillarFeatureNet + PointPillarsScatter +
SECOND/SECONDFPN + TransFusionHead) under the EntropySelector.  Head settings are those of
bevfusion/configs/nuscenes/det/transfusion/default.yaml with the pointpillars.yaml overrides: 384 input channels, a
512 x 512 grid, out_size_factor 4, 0.2 m voxels."""
_base_ = "bevfusion_pointpillars_spatial_temporal_feature.py"

model = dict(
    bbox_head=dict(
        _delete_=True,                  # the base builds the embedding-only graph (bbox_head=None)
        type="TransFusionHead", num_proposals=200, auxiliary=True, in_channels=384, hidden_channel=128, num_classes=10,
        num_decoder_layers=1, num_heads=8, nms_kernel_size=3, ffn_channel=256, dropout=0.1, bn_momentum=0.1,
        activation="relu", transpose_input=True,
        common_heads=dict(center=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2], vel=[2, 2]),
        test_cfg=dict(dataset="nuScenes", grid_size=[512, 512, 1], out_size_factor=4, voxel_size=[0.2, 0.2],
                      pc_range=[-51.2, -51.2], nms_type=None),
        bbox_coder=dict(pc_range=[-51.2, -51.2], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                        score_threshold=0.0, out_size_factor=4, voxel_size=[0.2, 0.2], code_size=10)),
)

selector = dict(
    type="EntropySelector",
    budget=4800,
    buffer_file="data/buffers/bevfusion_pointpillars_entropy.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
