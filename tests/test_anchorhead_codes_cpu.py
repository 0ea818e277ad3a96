"""CPU suite of the anchor head's direction classifier and scalar / 7-dim box codes: the builder and its remaining guards, the
state-dict names, the fused channel order, the committed goldens' distance to every float32 edge, the numpy restatement
(tests/anchorhead_codes.py) against the reference's own ``MultiGroupHead.predict`` (tests/golden/head_predict_codes.npz), the
planted edges' expectation, and the C entry's refusals (checked before any launch, so no GPU is needed)."""
import numpy as np
import pytest
import torch

import anchorhead_codes as AX

TASKS = [dict(num_class=1, class_names=["car"]), dict(num_class=2, class_names=["motorcycle", "bicycle"])]
AUX = dict(type="WeightedSoftmaxClassificationLoss", name="direction_classifier", loss_weight=0.2)
NMS = dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=64, nms_post_max_size=16, nms_iou_threshold=0.2)


def _head(n_dim=7, vec=False, loss_aux=AUX, **kw):
    from al3d.models.bbox_heads import MultiGroupHead
    from al3d.models.box_coder import GroundBox3dCoderTorch
    return MultiGroupHead(in_channels=16, tasks=TASKS, box_coder=GroundBox3dCoderTorch(False, vec, n_dim=n_dim),
                          loss_aux=loss_aux, **kw)


def test_loss_aux_builds_the_direction_classifier():
    from al3d.models.bbox_heads import Head
    h = Head(16, 14, 2, use_dir=True, num_dir=4)
    assert tuple(h.conv_dir.weight.shape) == (4, 16, 1, 1)
    m = _head(direction_offset=0.78)
    assert m.use_direction_classifier and m.direction_offset == 0.78 and m.box_n_dim == 7 and m.anchor_dim == 7
    assert [t.conv_dir.out_channels for t in m.tasks] == [4, 8]
    assert not hasattr(_head(loss_aux=None).tasks[0], "conv_dir")
    for n_dim, vec in ((7, False), (7, True), (9, False), (9, True)):
        m = _head(n_dim, vec)
        assert m.box_n_dim == n_dim + int(vec) and m._codes_entry
        assert [t.conv_box.out_channels for t in m.tasks] == [2 * m.box_n_dim, 4 * m.box_n_dim]
    # the CBGS form keeps its own entry point; any other code, or a classifier, takes the new one
    assert not _head(9, True, loss_aux=None)._codes_entry and _head(9, False, loss_aux=None)._codes_entry
    # linear_dim / norm_velo never reach the reference's decode: accepted
    from al3d.models.bbox_heads import MultiGroupHead
    from al3d.models.box_coder import GroundBox3dCoderTorch
    MultiGroupHead(in_channels=16, tasks=TASKS, box_coder=GroundBox3dCoderTorch(True, False, n_dim=9, norm_velo=True))


def test_config_builds_through_the_registry():
    import os
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "active",
                                       "pointpillars_mghead_entropy.py"))
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    h = m.bbox_head
    assert type(m).__name__ == "PointPillars" and h.use_direction_classifier and h.box_n_dim == 9 and not h.vec_encode
    assert len(h.tasks) == 6 and h._ch == sum(2 * n * 9 + 2 * n * n + 2 * n * 2 for n in h.num_classes)
    assert cfg.selector.type == "EntropySelector"


def test_refused_settings_name_themselves():
    with pytest.raises(NotImplementedError, match='mode="bev"'):
        _head(mode="bev")
    with pytest.raises(NotImplementedError, match="encode_background_as_zeros=False"):
        _head(encode_background_as_zeros=False)
    m = _head()
    ex = {"anchors": [torch.zeros((1, 8, 7)), torch.zeros((1, 16, 7))]}
    preds = [{"_fused": torch.zeros((1, 2, 2, m._ch))}]
    cfg = dict(score_threshold=0.1, post_center_limit_range=[-1, -1, -1, 1, 1, 1])
    with pytest.raises(NotImplementedError, match="use_rotate_nms=False"):
        m.predict(ex, preds, dict(cfg, nms=dict(NMS, use_rotate_nms=False)))
    with pytest.raises(NotImplementedError, match="use_multi_class_nms=True"):
        m.predict(ex, preds, dict(cfg, nms=dict(NMS, use_multi_class_nms=True)))


def test_state_dict_round_trip_with_conv_dir():
    m = _head(9, False)
    names = sorted(m.state_dict())
    assert names == sorted(f"tasks.{t}.conv_{k}.{p}" for t in range(2) for k in ("box", "cls", "dir") for p in ("weight", "bias"))
    g = torch.Generator().manual_seed(3)
    sd = {k: torch.randn(v.shape, generator=g) for k, v in m.state_dict().items()}
    m2 = _head(9, False)
    m2.load_state_dict(sd, strict=True)
    assert all(torch.equal(m2.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError, match="conv_dir"):
        _head(9, False, loss_aux=None).load_state_dict(sd, strict=True)


def test_fused_channel_offsets_of_the_two_task_head():
    m = _head(7, False)                               # box 2*7, 4*7 | cls 2*1, 4*2 | dir 2*2, 4*2
    assert (m._box_off, m._cls_off, m._dir_off, m._ch) == ([0, 14], [42, 44], [52, 56], 64)
    m = _head(9, True)
    assert (m._box_off, m._cls_off, m._dir_off, m._ch) == ([0, 20], [60, 62], [70, 74], 82)
    m = _head(9, True, loss_aux=None)
    assert (m._box_off, m._cls_off, m._dir_off, m._ch) == ([0, 20], [60, 62], [-1, -1], 70)
    # the helper that lays the goldens out for the library uses the head's order
    c = AX.load("s7_dir")
    hout, box_off, cls_off, dir_off = AX.fused(c)
    h = _head(7, False)
    assert (box_off, cls_off, dir_off, hout.shape[2]) == (h._box_off, h._cls_off, h._dir_off, h._ch)


def test_golden_cases_are_the_ones_asked_for():
    got = {n: (c["n_dim"], c["vec"], c["with_dir"], c["offset"]) for n, c in ((n, AX.load(n)) for n in AX.case_names())}
    assert got == {"s7_dir": (7, 0, True, 0.78), "s9_dir": (9, 0, True, 0.0), "v7_dir": (7, 1, True, 0.78),
                   "s9_nodir": (9, 0, False, 0.0), "v9_dir": (9, 1, True, 0.0)}
    c = AX.load("s7_dir")
    assert (c["B"], c["H"], c["W"], c["nc"], c["na"]) == (2, 8, 8, [1, 2], [2, 4])
    assert (c["params"]["pre_max"], c["params"]["post_max"]) == (64, 16)


@pytest.mark.parametrize("name", ["s7_dir", "s9_dir", "v7_dir", "s9_nodir", "v9_dir"])
def test_goldens_keep_clear_of_every_float32_edge(name):
    b = AX.bands(AX.load(name))
    print(name, {k: v for k, v in b.items()})
    assert b["score_gap"] >= 1e-5 - 1e-7 and b["score_thr"] >= 1e-4 - 1e-7      # recomputed in float64: one float32 ulp of slack
    assert b["angle"] >= 1e-3 - 1e-6 and b["dir"] >= 1e-3
    assert b["iou"] >= b["iou_delta"]
    assert b["cuts"] and b["empty"] == [(1, 1)]


@pytest.mark.parametrize("name", ["s7_dir", "s9_dir", "v7_dir", "s9_nodir", "v9_dir"])
def test_numpy_restatement_equals_the_reference_head(name):
    c = AX.load(name)
    got = AX.predict(c)
    flips = 0
    for b in range(c["B"]):
        assert len(c["ref"][b]["labels"]) > 5 and c["ref"][b]["boxes"].shape[1] == c["n_dim"]
        AX.assert_close(got[b], c["ref"][b], f"{name} sample {b}")
    if c["with_dir"]:                                 # the fix-up did something: without it the angles differ by pi somewhere
        plain = AX.predict(c, AX.fused(c, with_dir=False))
        for b in range(c["B"]):
            d = np.abs(plain[b]["boxes"][:, -1] - c["ref"][b]["boxes"][:, -1])
            flips += int((np.abs(d - np.pi) < 1e-5).sum())
            assert np.all((d < 1e-5) | (np.abs(d - np.pi) < 1e-5))
        assert flips > 3
    # padding and an odd record width do not move anything
    odd = AX.odd_layout(c)
    assert odd[0].shape[2] % 2 == 1
    for b in range(c["B"]):
        AX.assert_close(AX.predict(c, odd)[b], c["ref"][b], f"{name} padded sample {b}")


@pytest.mark.parametrize("n_dim,offset", [(7, 0.78), (9, 0.78), (7, 0.0)])
def test_planted_edges_expectation(n_dim, offset):
    """What torch computes for the plants, spelled out where the rule is the point of the plant."""
    _, _, plants = AX.edge_case(n_dim, offset)
    r, opp, mask = AX.edge_expected(plants, offset, n_dim)
    want = {"r==off label1": True, "r==off label0": False, "equal logits r>off": True, "equal logits r<off": False,
            "[nan,x]": True, "[x,nan]": False, "[nan,nan]": False, "r=off+ulp label0": True, "r=off+ulp label1": False,
            "r=off-ulp label0": False, "r=off-ulp label1": True, "z==range[5] flipped": True, "z>range[5] flipped": True,
            "z==range[5] kept angle": False, "-inf logit": True}
    assert {p[0]: bool(o) for p, o in zip(plants, opp)} == want
    assert [p[0] for p, m in zip(plants, mask) if not m] == ["z>range[5] flipped"]
    labels = AX.dir_labels(np.stack([p[3] for p in plants]))
    ra = np.array([p[2] for p in plants])
    mine = AX.fixup(ra.astype(np.float64), labels, offset)
    assert np.allclose(mine, r, atol=3e-7)


def test_codes_entry_refusals_come_before_any_launch():
    from al3d import lib
    want = {"n_dim 8": "n_dim must be 7 or 9", "n_dim 10": "n_dim must be 7 or 9", "dir in box window": "overlaps its box window",
            "dir in class window": "overlaps its class window", "dir straddles class start": "overlaps its class window",
            "dir past CH": "direction window exceeds CH", "mixed -1 first": "mixes -1", "mixed -1 second": "mixes -1"}
    got = AX.refusals()
    assert [g[0] for g in got] == list(want)
    for name, rc, msg in got:
        assert rc == -1, (name, rc, msg)                      # AL3D_EINVAL
        assert want[name] in msg and msg.startswith("al3d_head_decode_nms_codes:"), (name, msg)
    so = lib.load()
    import ctypes
    p = ctypes.c_void_p(4096)
    assert so.al3d_box_decode_codes_f32(p, p, 4, 8, 0, p, None) == -1 and b"n_dim must be 7 or 9" in so.al3d_last_error()
    assert so.al3d_box_decode_codes_f32(p, p, 4, 7, 2, p, None) == -1 and b"vec_encode" in so.al3d_last_error()
    assert so.al3d_box_decode_codes_f32(None, None, 0, 7, 0, None, None) == 0
