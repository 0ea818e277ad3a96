"""EntropySelector on det3d's plain CBGS VoxelNet: VoxelFeatureExtractorV3 + SpMiddleResNetFHD + RPN + MultiGroupHead
-- the model of the reference's ``examples/active/cbgs_full.py``.  ``SpMiddleResNetFHD`` is the residual encoder of
``_cbgs_common.py`` without the FPN taps; it returns the dense map alone.  Everything else is the shared part."""
_base_ = "_cbgs_common.py"

model = dict(
    type="VoxelNet",
    backbone=dict(_delete_=True, type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8, norm_cfg=None),
)

selector = dict(
    type="EntropySelector",
    budget=4800,
    buffer_file="data/buffers/voxelnet_cbgs_entropy.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
