"""CPU suite: det3d's single-stage sparse encoders SpMiddleFHD / SpMiddleResNetFHD (reference
det3d/models/backbones/scn.py:100-205, 395-457) -- registry names, the reference's ``middle_conv.<i>`` state-dict keys,
the layer plan -- and the two example configs that use them."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RES_CONVS = {0: (5, 16, (3, 3, 3)), 5: (16, 32, (3, 3, 3)), 10: (32, 64, (3, 3, 3)), 15: (64, 128, (3, 3, 3)),
             20: (128, 128, (3, 1, 1))}
RES_BLOCKS = {3: 16, 4: 16, 8: 32, 9: 32, 13: 64, 14: 64, 18: 128, 19: 128}
FHD_CHANNELS = [16, 16, 32, 32, 32, 64, 64, 64, 64, 64, 64, 64, 64, 64]


def _bn_keys(prefix):
    return [f"{prefix}.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]


def test_registry_resolves_the_reference_encoder_names():
    from al3d.models import BACKBONES
    from al3d.models.backbones import _SparseEncoderBase
    for name in ("SpMiddleFHD", "SpMiddleResNetFHD"):
        cls = BACKBONES.get(name)
        assert cls is not None and issubclass(cls, _SparseEncoderBase), name
        assert hasattr(cls, "rulebook_for")


def test_spmiddle_resnet_fhd_state_dict():
    from al3d.models import build_backbone
    m = build_backbone(dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8, norm_cfg=None))
    want, shapes = [], {}
    for i in range(23):
        if i in RES_CONVS:
            cin, cout, k = RES_CONVS[i]
            want.append(f"middle_conv.{i}.weight")
            shapes[want[-1]] = (*k, cin, cout)
            want += _bn_keys(f"middle_conv.{i + 1}")
        elif i in RES_BLOCKS:
            c = RES_BLOCKS[i]
            for j in (1, 2):
                want += [f"middle_conv.{i}.conv{j}.weight", f"middle_conv.{i}.conv{j}.bias"]
                shapes[f"middle_conv.{i}.conv{j}.weight"] = (3, 3, 3, c, c)
    sd = m.state_dict()
    assert sorted(k for k in sd if sd[k].dim() == 5) == sorted(shapes)
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k
    for i, c in RES_BLOCKS.items():
        for j in (1, 2):
            for k in _bn_keys(f"middle_conv.{i}.bn{j}"):
                assert k in sd, k
            assert tuple(sd[f"middle_conv.{i}.conv{j}.bias"].shape) == (c,)
    for i in RES_CONVS:
        assert f"middle_conv.{i}.bias" not in sd
        for k in _bn_keys(f"middle_conv.{i + 1}"):
            assert k in sd, k
    assert all(k.startswith("middle_conv.") for k in sd)
    # the same tensors as the FPN encoder, stage by stage: its parameters copy over by position
    fpn = build_backbone(dict(type="FPNSpMiddleResNetFHD", num_input_features=5, ds_factor=8, norm_cfg=None))
    assert [tuple(v.shape) for v in fpn.state_dict().values()] == [tuple(v.shape) for v in sd.values()]
    bn = m.middle_conv[1]
    assert bn.eps == 1e-3 and bn.momentum == 0.01


def test_spmiddle_fhd_state_dict_and_layers():
    from al3d.models import build_backbone
    m = build_backbone(dict(type="SpMiddleFHD", num_input_features=128, ds_factor=8, norm_cfg=None))
    sd = m.state_dict()
    want, cin = [], 128
    for li, cout in enumerate(FHD_CHANNELS):
        i = 3 * li
        want.append(f"middle_conv.{i}.weight")
        k = (3, 1, 1) if li == 13 else (3, 3, 3)
        assert tuple(sd[f"middle_conv.{i}.weight"].shape) == (*k, cin, cout), i
        want += _bn_keys(f"middle_conv.{i + 1}")
        cin = cout
    assert list(sd) == want
    convs = [m.middle_conv[3 * li] for li in range(14)]
    strided = [c for c in convs if not c.subm]
    assert [convs.index(c) for c in strided] == [2, 5, 9, 13]
    assert [c.stride for c in strided] == [(2, 2, 2)] * 3 + [(2, 1, 1)]
    assert [c.padding for c in strided] == [(1, 1, 1), (1, 1, 1), (0, 1, 1), (0, 0, 0)]
    assert strided[-1].kernel_size == (3, 1, 1)
    assert all(c.bias is None for c in convs)


def test_layer_plan_and_output_shape():
    """One stage; 21 / 14 conv layers; the last level of a [96, 88, 40] grid is 2 x 11 x 12."""
    from al3d.models import build_backbone
    for name, nin, layers, cout in (("SpMiddleResNetFHD", 5, 21, 128), ("SpMiddleFHD", 128, 14, 64)):
        m = build_backbone(dict(type=name, num_input_features=nin)).eval()
        assert len(m._stages()) == 1
        from al3d.models.backbones import SparseBasicBlock, _SpConvParams
        convs = []
        for mod in m.middle_conv.children():
            if isinstance(mod, _SpConvParams):
                convs.append(mod)
            elif isinstance(mod, SparseBasicBlock):
                convs += [mod.conv1, mod.conv2]
        assert len(convs) == layers and convs[-1].out_channels == cout
        shape = [41, 88, 96]
        for c in convs:
            if not c.subm:
                shape = m._out_shape(shape, c.kernel_size, c.stride, c.padding)
        assert shape == [2, 11, 12]


@pytest.mark.parametrize("name,reader,backbone", [
    ("voxelnet_cbgs_entropy.py", "VoxelFeatureExtractorV3", "SpMiddleResNetFHD"),
    ("second_vfe_entropy.py", "VoxelFeatureExtractor", "SpMiddleFHD")])
def test_example_configs_build(name, reader, backbone):
    from al3d.models import build_detector
    from al3d.models.readers import needs_point_slots
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", name))
    assert cfg.model.type == "VoxelNet" and cfg.selector.type == "EntropySelector"
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    assert type(m.reader).__name__ == reader and type(m.backbone).__name__ == backbone
    assert needs_point_slots(cfg.model.reader) == (reader == "VoxelFeatureExtractor")
    if reader == "VoxelFeatureExtractor":
        assert m.backbone.middle_conv[0].in_channels == 128 and m.reader.out_channels == 128


def test_detector_asks_for_point_slots():
    """A learned reader cannot take the voxelizer's mean: without ``voxels`` the detector says how to get them."""
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "second_vfe_entropy.py"))
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg).eval()
    ex = dict(voxel_features=torch.zeros(4, 5), coordinates=torch.zeros(4, 4, dtype=torch.int32),
              num_voxels=torch.tensor([4]), shape=[[96, 88, 40]])
    with pytest.raises(RuntimeError, match="with_points=True"):
        m.sparse_stage(ex)
