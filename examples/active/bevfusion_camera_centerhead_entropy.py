"""BEVFusion camera-only detector (Swin-T -> GeneralizedLSSFPN -> LSSTransform -> GeneralizedResNet -> LSSFPN ->
CenterHead) under the EntropySelector.  Numbers of bevfusion/configs/nuscenes/det/centerhead/lssfpn/camera/256x704/swint/
default.yaml and the defaults it inherits (centerhead/default.yaml, lssfpn/camera/default.yaml): 0.4 m BEV cells over
+-51.2 m, 0.5 m depth bins, view-transform downsample 2, per-task NMS types and scales.  The decoder keeps the view
transform's [x, y] maps, so the head is built with transpose_input=False."""
_base_ = "bevfusion_camera_lidar_spatial_temporal_feature.py"

image_size = [256, 704]
model = dict(
    _delete_=True,
    type="BEVFusionCameraOnly",
    camera=dict(
        backbone=dict(type="SwinTransformer", embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7,
                      mlp_ratio=4, qkv_bias=True, patch_norm=True, out_indices=[1, 2, 3]),
        neck=dict(type="GeneralizedLSSFPN", in_channels=[192, 384, 768], out_channels=256, start_level=0, num_outs=3,
                  upsample_cfg=dict(mode="bilinear", align_corners=False)),
        vtransform=dict(type="LSSTransform", in_channels=256, out_channels=80, image_size=image_size, feature_size=[32, 88],
                        xbound=[-51.2, 51.2, 0.4], ybound=[-51.2, 51.2, 0.4], zbound=[-10.0, 10.0, 20.0],
                        dbound=[1.0, 60.0, 0.5], downsample=2)),
    decoder=dict(
        backbone=dict(type="GeneralizedResNet", in_channels=80, blocks=[[2, 128, 2], [2, 256, 2], [2, 512, 1]]),
        neck=dict(type="LSSFPN", in_indices=[-1, 0], in_channels=[512, 128], out_channels=256, scale_factor=2)),
    bbox_head=dict(
        type="CenterHead", in_channels=256, share_conv_channel=64, norm_bbox=True, transpose_input=False,
        tasks=[["car"], ["truck", "construction_vehicle"], ["bus", "trailer"], ["barrier"], ["motorcycle", "bicycle"],
               ["pedestrian", "traffic_cone"]],
        common_heads=dict(reg=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2], vel=[2, 2]),
        separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3),
        test_cfg=dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_per_img=500, max_pool_nms=False,
                      min_radius=[4, 12, 10, 1, 0.85, 0.175], score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1],
                      nms_type=["circle", "rotate", "rotate", "circle", "rotate", "rotate"],
                      nms_scale=[[1.0], [1.0, 1.0], [1.0, 1.0], [1.0], [1.0, 1.0], [2.5, 4.0]],
                      pre_max_size=1000, post_max_size=83, nms_thr=0.2),
        bbox_coder=dict(type="CenterPointBBoxCoder", pc_range=[-51.2, -51.2], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                        max_num=500, score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9)),
)

selector = dict(
    type="EntropySelector",
    budget=4800,
    buffer_file="data/buffers/bevfusion_camera_centerhead_entropy.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
