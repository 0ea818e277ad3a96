"""EntropySelector on a SECOND model: VoxelFeatureExtractor (two VFE layers + a 128 x 128 linear, one fused launch on the
padded point slots) + SpMiddleFHD + RPN + MultiGroupHead under ``VoxelNet``.  The reader reads ``voxels`` /
``num_points``: the tools build the loader with ``with_points=True`` from the reader's ``needs_point_slots``.  The encoder
takes the reader's 128 channels and gives a 64 * 2 = 128-channel map; tasks, anchors and the rest are those of
``_cbgs_common.py``."""
_base_ = "_cbgs_common.py"

model = dict(
    type="VoxelNet",
    reader=dict(_delete_=True, type="VoxelFeatureExtractor", num_input_features=5, use_norm=True, num_filters=[32, 128],
                with_distance=False),
    backbone=dict(_delete_=True, type="SpMiddleFHD", num_input_features=128, ds_factor=8, norm_cfg=None),
    neck=dict(num_input_features=128),
)

selector = dict(
    type="EntropySelector",
    budget=4800,
    buffer_file="data/buffers/second_vfe_entropy.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
