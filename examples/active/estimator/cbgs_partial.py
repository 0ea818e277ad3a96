"""Active-learning selection config: EntropySelector on the CBGS FPNVoxelNet whose detections are rescored by the box-wise
IoU Estimator before the selector reads them -- the frames picked are those whose boxes the model itself believes are
badly placed (same keys as the reference's examples/active/cbgs_partial.py; see ../_cbgs_common.py for the shared part).

The estimator runs only when its weights are given: ``tools/active_select.py --estimator-checkpoint FILE`` or
``estimator_load_from`` below; without them the detector's own scores are used."""
_base_ = "../_cbgs_common.py"

# the six CBGS task groups of _cbgs_common.py (a config cannot read its base's names); the estimator takes the one-hot
# width, 10, from them
_GROUPS = [["car"], ["truck", "construction_vehicle"], ["bus", "trailer"], ["barrier"], ["motorcycle", "bicycle"],
           ["pedestrian", "traffic_cone"]]

estimator = dict(
    type="Estimator",
    tasks=[dict(num_class=len(g), class_names=g) for g in _GROUPS],
    dim_feat=224,           # accepted and unused, as in the reference (its feature interpolation is commented out)
)
estimator_load_from = None

selector = dict(
    type="EntropySelector",
    budget=4800,
    buffer_file="data/buffers/partial_entropy.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
