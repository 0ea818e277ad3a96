"""Active-learning selection config: CaldSelector on the CBGS FPNVoxelNet (same keys as the
reference's examples/active/cbgs_cald.py; see _cbgs_common.py for the shared part)."""
_base_ = "_cbgs_common.py"

selector = dict(
    type="CaldSelector",
    budget=4800,
    buffer_file="data/buffers/cald.json",
    infos_origin="data/nuScenes/infos_train_10sweeps_withvelo.pkl",
)
# The two rankings CaldSelector replays (buffer_path, jsdiv_path) come from tools/active_prepass.py --mode cald, or from the
# selector itself when it is given a detector and a dataloader (tools/active_select.py --pred):
#   selector.update(prepass=True, prepass_view=(True, False, 0.0, 1.0),        # flip_x, flip_y, rot, scale
#                   buffer_path="data/buffers/cald_ent_sorted_idx.json", jsdiv_path="data/buffers/idx_to_jsdiv.pkl")
