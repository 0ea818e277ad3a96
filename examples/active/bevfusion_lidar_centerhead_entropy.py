"""BEVFusion lidar-only detector (voxelnet_0p075 encoder + SECOND/SECONDFPN) with CenterPoint's CenterHead under the
EntropySelector: bevfusion/mmdet3d/models/heads/bbox/centerpoint.py:249-884 feeding
det3d/selectors/entropy_selector.py:50-86.  Head settings are those of
bevfusion/configs/nuscenes/det/centerhead/default.yaml on the 180 x 180 map of the lidar branch."""
_base_ = "bevfusion_lidar_spatial_temporal_feature.py"

model = dict(
    bbox_head=dict(
        _delete_=True,                  # the base builds the embedding-only graph (bbox_head=None)
        type="CenterHead", in_channels=512, share_conv_channel=64, norm_bbox=True, transpose_input=True,
        tasks=[["car"], ["truck", "construction_vehicle"], ["bus", "trailer"], ["barrier"], ["motorcycle", "bicycle"],
               ["pedestrian", "traffic_cone"]],
        common_heads=dict(reg=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2], vel=[2, 2]),
        separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3),
        test_cfg=dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_per_img=500, max_pool_nms=False,
                      min_radius=[4, 12, 10, 1, 0.85, 0.175], score_threshold=0.1, out_size_factor=8, voxel_size=[0.075, 0.075],
                      nms_type="rotate", pre_max_size=1000, post_max_size=83, nms_thr=0.2),
        bbox_coder=dict(type="CenterPointBBoxCoder", pc_range=[-54.0, -54.0], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                        max_num=500, score_threshold=0.1, out_size_factor=8, voxel_size=[0.075, 0.075], code_size=9)),
)

selector = dict(
    type="EntropySelector",
    budget=4800,
    buffer_file="data/buffers/bevfusion_lidar_centerhead_entropy.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
