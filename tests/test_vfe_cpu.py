"""CPU suite: det3d's VFE readers -- registry names, the reference's state-dict keys and shapes, the float64
restatement (tests/vfe_fp64.py) against the reference's own outputs (tests/golden/vfe_readers.npz, written by
tools/gen_golden_vfe.py), and the argument checks of al3d_vfe_net_f32, which run in front of any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import vfe_fp64 as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "vfe_readers.npz"))
CASES = [str(c) for c in G["cases"]]


def _config(tag):
    c = [int(v) for v in G[f"{tag}.config"]]
    return dict(kind=tag.split("_")[0], use_norm=bool(c[0]), wd=bool(c[1]), F=c[2], T=c[3], filters=c[4:])


def _params(tag):
    pre = tag + "."
    skip = ("out", "keys", "shapes", "config")
    return {k[len(pre):]: G[k] for k in G.files if k.startswith(pre) and k[len(pre):] not in skip}


def _prefixes(cfg):
    if cfg["kind"] == "vfe":
        return [("vfe1.linear", "vfe1.norm"), ("vfe2.linear", "vfe2.norm"), ("linear", "norm")]
    return [(f"vfe_layers.{i}.linear", f"vfe_layers.{i}.norm") for i in range(len(cfg["filters"]))] + [("linear", "norm")]


def _build(cfg):
    from al3d.models import build_reader
    return build_reader(dict(type="VoxelFeatureExtractor" if cfg["kind"] == "vfe" else "VoxelFeatureExtractorV2",
                             num_input_features=cfg["F"], use_norm=cfg["use_norm"], num_filters=cfg["filters"],
                             with_distance=cfg["wd"]))


def test_registry_resolves_the_reference_reader_names():
    from al3d.models import READERS
    for name in ("VFELayer", "VoxelFeatureExtractor", "VoxelFeatureExtractorV2", "SimpleVoxel", "VFEV3_ablation",
                 "VoxelFeatureExtractorV3"):
        assert READERS.get(name) is not None, name


def test_readers_say_what_they_need_from_the_loader():
    from al3d.models import READERS
    from al3d.models.readers import needs_point_slots
    for name in ("VoxelFeatureExtractor", "VoxelFeatureExtractorV2", "SimpleVoxel", "VFEV3_ablation", "PillarFeatureNet"):
        assert READERS.get(name).needs_point_slots and not READERS.get(name).mean_reader, name
        assert needs_point_slots(dict(type=name))
    assert not READERS.get("VoxelFeatureExtractorV3").needs_point_slots and READERS.get("VoxelFeatureExtractorV3").mean_reader
    assert not needs_point_slots(dict(type="VoxelFeatureExtractorV3")) and not needs_point_slots(None)
    assert not needs_point_slots(dict(type="DynamicPillarFeatureNet"))


@pytest.mark.parametrize("tag", CASES)
def test_state_dict_is_the_references(tag):
    """Keys in the reference's order, shapes equal, and the golden parameters load with strict=True."""
    mod = _build(_config(tag))
    sd = mod.state_dict()
    assert list(sd) == [str(k) for k in G[f"{tag}.keys"]]
    assert [str(tuple(sd[k].shape)) for k in sd] == [str(s) for s in G[f"{tag}.shapes"]]
    state = {k: torch.from_numpy(np.asarray(v)) for k, v in _params(tag).items()}
    for k in sd:
        if k.endswith("num_batches_tracked"):
            state[k] = sd[k]
    mod.load_state_dict(state, strict=True)
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            assert m.eps == 1e-3 and m.momentum == 0.01


def test_small_readers_and_vfelayer_state_dicts():
    from al3d.models import build_reader
    for name, key in (("SimpleVoxel", "simple"), ("VFEV3_ablation", "ablation")):
        sd = build_reader(dict(type=name)).state_dict()
        assert list(sd) == [str(k) for k in G[f"{key}.keys"]]
    sd = build_reader(dict(type="VFELayer", in_channels=8, out_channels=32)).state_dict()
    assert list(sd) == [str(k) for k in G["vfelayer.keys"]]
    assert [str(tuple(sd[k].shape)) for k in sd] == [str(s) for s in G["vfelayer.shapes"]]
    sd = build_reader(dict(type="VFELayer", in_channels=8, out_channels=32, use_norm=False)).state_dict()
    assert list(sd) == ["linear.weight", "linear.bias"]


def test_v2_with_three_layers_raises_clearly():
    from al3d.models import build_reader
    mod = build_reader(dict(type="VoxelFeatureExtractorV2", num_filters=[32, 64, 128])).eval()
    with pytest.raises(NotImplementedError, match="one or two"):
        mod.net("cpu")


def test_readers_refuse_host_tensors_and_training():
    from al3d import lib
    from al3d.models import build_reader
    mod = build_reader(dict(type="VoxelFeatureExtractor", num_input_features=5)).eval()
    with pytest.raises(lib.Al3dError, match="device tensors"):
        mod(torch.zeros(2, 10, 5), torch.ones(2, dtype=torch.int32))
    for name in ("SimpleVoxel", "VFEV3_ablation"):
        with pytest.raises(lib.Al3dError, match="device tensors"):
            build_reader(dict(type=name))(torch.zeros(2, 10, 4), torch.ones(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="eval"):
        mod.train().net("cpu")


@pytest.mark.parametrize("tag", CASES)
def test_fp64_restatement_matches_reference_readers(tag):
    """The reference ran in f32 on the CPU: 1e-6 of the output's magnitude.  Anything looser means the restatement (the
    padded-slot rule, the fold, the order of mask and max) is wrong."""
    cfg = _config(tag)
    vox, num = G[f"voxels_F{cfg['F']}_T{cfg['T']}"], G[f"num_points_F{cfg['F']}_T{cfg['T']}"]
    ref, absum = V.vfe_net(vox, num, V.fold_layers(_params(tag), _prefixes(cfg)), cfg["wd"])
    out = G[f"{tag}.out"]
    assert ref.shape == out.shape and (absum > 0).all()
    assert np.abs(out - ref).max() <= 1e-6 * np.abs(ref).max()
    assert (np.abs(out - ref) <= 2 * V.bound(cfg["T"], [w.shape[1] for w, _, _ in
                                                        V.fold_layers(_params(tag), _prefixes(cfg))]) * absum).all()


def test_golden_tells_the_padded_slot_rule_apart():
    """Masking the padded slots in front of vfe1 (PillarFeatureNet's order) moves the default case's output."""
    tag = CASES[0]
    cfg = _config(tag)
    vox, num = G[f"voxels_F{cfg['F']}_T{cfg['T']}"], G[f"num_points_F{cfg['F']}_T{cfg['T']}"]
    wrong, _ = V.vfe_net(vox, num, V.fold_layers(_params(tag), _prefixes(cfg)), cfg["wd"], pad_in_max1=False)
    out = G[f"{tag}.out"]
    moved = np.abs(wrong - out).max(1) > 1e-3 * np.abs(out).max(1)
    assert moved[num < cfg["T"]].mean() >= 0.1 and not moved[num == cfg["T"]].any()


def _call(so, M=0, T=10, F=5, wd=0, U1=16, w2=8, U2=64, C=128, vpw=None, blocks=0, ptr=8, w1=8, out=None):
    p = ctypes.c_void_p
    args = [p(ptr), p(ptr), M, T, F, wd, p(w1), p(8), p(8), U1, p(w2) if w2 else None, p(8) if w2 else None,
            p(8) if w2 else None, U2, p(8), p(8), p(8), C, p(out) if out else None]
    if vpw is None:
        return so.al3d_vfe_net_f32(*args, None)
    return so.al3d_vfe_net_launch_f32(*args, vpw, blocks, None)


def test_bad_arguments_fail_without_gpu():
    """Every limit of the entry point is refused with the project's error code in front of any launch; M == 0 with good
    sizes launches nothing and succeeds."""
    from al3d import lib
    so = lib.load()
    assert _call(so) == 0 and _call(so, vpw=0) == 0 and _call(so, vpw=3, blocks=2) == 0
    assert _call(so, w2=0, U1=32, U2=0, C=64) == 0                      # one VFE layer
    bad = [dict(T=0), dict(T=65), dict(F=2), dict(F=11), dict(U1=8), dict(U1=24), dict(U1=80), dict(U2=8),
           dict(U2=72), dict(U2=128, C=256), dict(C=64), dict(C=130), dict(w2=0, U1=32, U2=0, C=128), dict(M=-1),
           dict(w1=0), dict(vpw=-1), dict(vpw=17), dict(vpw=0, blocks=-1), dict(M=4, ptr=0), dict(M=4)]
    for kw in bad:
        assert _call(so, **kw) == -1, kw
        assert so.al3d_last_error(), kw
    assert _call(so, T=65) == -1 and b"1 <= T <= 64" in so.al3d_last_error()
    assert _call(so, F=11) == -1 and b"3 <= F <= 10" in so.al3d_last_error()
    assert _call(so, U1=80) == -1 and b"multiple of 16 in [16, 64]" in so.al3d_last_error()
    assert _call(so, C=64) == -1 and b"twice the last VFE layer" in so.al3d_last_error()
    with pytest.raises(lib.Al3dError):
        lib.call("al3d_vfe_net_f32", None, None, 0, 10, 5, 0, None, None, None, 16, None, None, None, 0, None, None,
                 None, 32, None, None)
