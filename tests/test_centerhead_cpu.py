"""CPU: the registry builds ``CenterHead`` from the settings of the reference's ``det/centerhead/default.yaml``, its
parameters carry the reference's names, a reference-named state dict loads strictly, and unsupported settings raise."""
import ctypes
import os

import pytest
import torch

TASKS = [["car"], ["truck", "construction_vehicle"], ["bus", "trailer"], ["barrier"], ["motorcycle", "bicycle"],
         ["pedestrian", "traffic_cone"]]
COMMON = dict(reg=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2], vel=[2, 2])
CFG = dict(
    type="CenterHead", in_channels=512, tasks=TASKS, common_heads=COMMON, share_conv_channel=64, norm_bbox=True,
    train_cfg=dict(point_cloud_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], grid_size=[1024, 1024, 1], voxel_size=[0.075, 0.075, 0.2],
                   out_size_factor=8, dense_reg=1, gaussian_overlap=0.1, max_objs=500, min_radius=2,
                   code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]),
    test_cfg=dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_per_img=500, max_pool_nms=False,
                  min_radius=[4, 12, 10, 1, 0.85, 0.175], score_threshold=0.1, out_size_factor=8, voxel_size=[0.075, 0.075],
                  nms_type="rotate", pre_max_size=1000, post_max_size=83, nms_thr=0.2),
    bbox_coder=dict(type="CenterPointBBoxCoder", pc_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0],
                    post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=500, score_threshold=0.1, out_size_factor=8,
                    voxel_size=[0.075, 0.075], code_size=9),
    separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3),
    loss_cls=dict(type="GaussianFocalLoss", reduction="mean"), loss_bbox=dict(type="L1Loss", reduction="mean", loss_weight=0.25))


def reference_state_dict_shapes():
    """Names and shapes of the reference module tree (mmcv ConvModule: ``conv`` / ``bn``), written out from
    centerpoint.py:56-89,319-337 -- not read from the module under test."""
    def conv_module(prefix, cin, cout):
        return {f"{prefix}.conv.weight": (cout, cin, 3, 3), f"{prefix}.bn.weight": (cout,), f"{prefix}.bn.bias": (cout,),
                f"{prefix}.bn.running_mean": (cout,), f"{prefix}.bn.running_var": (cout,), f"{prefix}.bn.num_batches_tracked": ()}
    out = conv_module("shared_conv", 512, 64)
    for t, names in enumerate(TASKS):
        for head, classes in list((k, v[0]) for k, v in COMMON.items()) + [("heatmap", len(names))]:
            out.update(conv_module(f"task_heads.{t}.{head}.0", 64, 64))
            out[f"task_heads.{t}.{head}.1.weight"] = (classes, 64, 3, 3)
            out[f"task_heads.{t}.{head}.1.bias"] = (classes,)
    return out


def test_registry_builds_center_head_with_reference_names():
    from al3d.models import build_head
    head = build_head(dict(CFG))
    want = reference_state_dict_shapes()
    sd = head.state_dict()
    assert sorted(sd) == sorted(want)
    assert all(tuple(sd[k].shape) == want[k] for k in want)
    assert head.class_names == TASKS and head.num_classes == [1, 2, 2, 1, 2, 2]
    g = torch.Generator().manual_seed(0)
    ref = {k: (torch.tensor(7) if s == () else torch.randn(s, generator=g)) for k, s in want.items()}
    head.load_state_dict(ref, strict=True)
    assert torch.equal(head.task_heads[5].heatmap[1].bias, ref["task_heads.5.heatmap.1.bias"])
    assert float(build_head(dict(CFG)).task_heads[0].heatmap[1].bias.detach()[0]) == pytest.approx(-2.19)


def test_training_and_unbuilt_variants_raise():
    from al3d.models import build_head
    with pytest.raises(NotImplementedError):
        build_head(dict(CFG, separate_head=dict(type="DCNSeparateHead", dcn_config=dict(), init_bias=-2.19)))
    head = build_head(dict(CFG, common_heads=dict(reg=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2])))
    assert not any(".vel." in k for k in head.state_dict())
    head.train()
    with pytest.raises(RuntimeError):
        head(torch.zeros(1, 4, 4, 512))


def test_entry_points_validate_before_any_launch():
    from al3d import lib
    so = lib.load()
    I = ctypes.c_int
    one, chan = (I * 1)(1), (I * 6)(9, 0, 2, 3, 6, 7)
    f5, f6, f4, f1 = (ctypes.c_float * 5)(), (ctypes.c_float * 6)(), (ctypes.c_float * 4)(), (ctypes.c_float * 1)()
    args = lambda k, hw: (None, 0, hw, hw, 10, 1, 1, one, chan, k, 1, f5, 0.1, f6, (I * 1)(0), f4, f1, 0.1, 0.2, 1000, 83,  # noqa: E731
                          None, 1, None, None, None, None, None, None)
    assert so.al3d_center_decode_nms_f32(*args(500, 128)) == 0                 # B = 0: nothing to do
    assert so.al3d_center_decode_nms_f32(*args(500, 20)) == -1 and b"exceeds" in so.al3d_last_error()
    assert so.al3d_center_decode_nms_f32(*args(2000, 128)) == -1 and b"max_num" in so.al3d_last_error()
    rc = so.al3d_conv3x3_grouped_nhwc_f32(None, None, None, None, 0, 4, 4, 1, (I * 1)(9), (I * 1)(0), 9, None)
    assert rc == -1 and b"cout" in so.al3d_last_error()
    rc = so.al3d_conv3x3_grouped_nhwc_f32(None, None, None, None, 0, 4, 4, 1, (I * 1)(3), (I * 1)(7), 9, None)
    assert rc == -1 and b"outside" in so.al3d_last_error()


def test_example_config_builds():
    from al3d.models import build_detector
    from al3d.utils import Config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, "examples", "active", "bevfusion_lidar_centerhead_entropy.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    assert type(model.bbox_head).__name__ == "CenterHead" and model.bbox_head.transpose_input
    assert model.bbox_head.bbox_coder["max_num"] == 500 and cfg.selector.type == "EntropySelector"
