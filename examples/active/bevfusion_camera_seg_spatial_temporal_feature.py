"""BEVFusion camera-only map segmentation model (Swin-T -> GeneralizedLSSFPN -> LSSTransform -> GeneralizedResNet ->
LSSFPN -> BEVSegmentationHead) as the embedding model of the spatial-temporal-feature selector.  Numbers of
bevfusion/configs/nuscenes/seg/camera-bev256d2.yaml and the seg/default.yaml it inherits: 0.4 m BEV cells over +-51.2 m,
view-transform downsample 2, a 160 / 320 / 640-channel decoder whose 128 x 128 x 256 map of 0.8 m cells the head resamples
onto the 200 x 200 map grid of 0.5 m cells over +-50 m; six map classes.  No detection head (``heads.object: null``): the
sweep produces the [N,256] BEV embeddings, and every output dict holds ``masks_bev`` [6, 200, 200], ``map_entropy`` [6] and
``map_area`` [6].  The decoder keeps the view transform's [x, y] maps, so the head is built with transpose_input=False."""
_base_ = "bevfusion_camera_centerhead_entropy.py"

map_classes = ["drivable_area", "ped_crossing", "walkway", "stop_line", "carpark_area", "divider"]
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
        backbone=dict(type="GeneralizedResNet", in_channels=80, blocks=[[2, 160, 2], [2, 320, 2], [2, 640, 1]]),
        neck=dict(type="LSSFPN", in_indices=[-1, 0], in_channels=[640, 160], out_channels=256, scale_factor=2)),
    bbox_head=None,
    map_head=dict(
        type="BEVSegmentationHead", in_channels=256, transpose_input=False,
        grid_transform=dict(input_scope=[[-51.2, 51.2, 0.8], [-51.2, 51.2, 0.8]],
                            output_scope=[[-50, 50, 0.5], [-50, 50, 0.5]]),
        classes=map_classes, loss="focal"),
)

selector = dict(
    type="SpatialTemporalFeatureSelector",
    budget=4800,
    buffer_file="data/buffers/bevfusion_camera_seg_stf.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
