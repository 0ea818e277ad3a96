"""BEVFusion lidar-only branch (voxelnet_0p075) on DYNAMIC voxelization as the embedding model of the diversity
selector.  Same grid / voxel / channel settings as bevfusion_lidar_spatial_temporal_feature.py; the caps of -1 select
``detector_ops.DynamicVoxelizer`` -- the reference's ``voxelize.max_num_points <= 0`` branch
(bevfusion/mmdet3d/models/fusion_models/bevfusion.py:46-49: dynamic_voxelize, then DynamicScatter with mean).  Every
in-range point takes part, voxels come in (z, y, x) order, so the per-frame embedding and with it the selection do not
depend on the order of the points in the file, and no first-point grid stays resident.
No detection head: the sweep produces the [N,512] BEV embeddings only."""
_base_ = "_cbgs_common.py"

voxel_generator = dict(
    range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0],
    voxel_size=[0.075, 0.075, 0.2],
    max_points_in_voxel=-1,         # -1 / -1: no cap per voxel, no cap per frame
    max_voxel_num=-1,
)

model = dict(bbox_head=None)        # encoder + SECOND/SECONDFPN only (same modules as the CBGS model)

selector = dict(
    type="SpatialTemporalFeatureSelector",
    budget=4800,
    buffer_file="data/buffers/bevfusion_lidar_dynamic_stf.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
