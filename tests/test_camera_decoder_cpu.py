"""CPU suite of the camera-only BEV decoder: the three components and the detector build through the registries with the
reference's state-dict keys, and the float64 yardstick (tests/camera_decoder_fp64.py) is pinned -- LSSFPN and
LSSTransform.get_cam_feats to the reference's own output, BasicBlock to torch.nn float64 modules."""
import json
import os

import numpy as np
import torch
from torch import nn

import camera_decoder_fp64 as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bevfusion_camera_decoder.npz")
BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _bn(p):
    return {f"{p}.{k}" for k in BN}


def _block_keys(p, downsample):
    keys = {f"{p}.conv1.weight", f"{p}.conv2.weight"} | _bn(f"{p}.bn1") | _bn(f"{p}.bn2")
    if downsample:
        keys |= {f"{p}.downsample.0.weight"} | _bn(f"{p}.downsample.1")
    return keys


# GeneralizedResNet(80, [[2,128,2],[2,256,2],[2,512,1]]): the first block of every stage changes the channel count
RESNET_KEYS = set().union(*[_block_keys(f"{s}.{b}", b == 0) for s in range(3) for b in range(2)])
LSSFPN_KEYS = {"fuse.0.weight", "fuse.3.weight", "upsample.1.weight"} | _bn("fuse.1") | _bn("fuse.4") | _bn("upsample.2")
LSSTRANSFORM_KEYS = {"dx", "bx", "nx", "frustum", "depthnet.weight", "depthnet.bias"} | \
    {f"downsample.{i}.weight" for i in (0, 3, 6)} | _bn("downsample.1") | _bn("downsample.4") | _bn("downsample.7")

RESNET_CFG = dict(type="GeneralizedResNet", in_channels=80, blocks=[[2, 128, 2], [2, 256, 2], [2, 512, 1]])
LSSFPN_CFG = dict(type="LSSFPN", in_indices=[-1, 0], in_channels=[512, 128], out_channels=256, scale_factor=2)


def detector_cfg(image_size=(64, 96), grid=32, bbox_head=None, grid_y=None):
    half, half_y = grid * 0.4 / 2, (grid if grid_y is None else grid_y) * 0.4 / 2
    return dict(
        type="BEVFusionCameraOnly",
        camera=dict(
            backbone=dict(type="SwinTransformer", embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7,
                          mlp_ratio=4, qkv_bias=True, patch_norm=True, out_indices=[1, 2, 3]),
            neck=dict(type="GeneralizedLSSFPN", in_channels=[192, 384, 768], out_channels=256, start_level=0, num_outs=3,
                      upsample_cfg=dict(mode="bilinear", align_corners=False)),
            vtransform=dict(type="LSSTransform", in_channels=256, out_channels=80, image_size=list(image_size),
                            feature_size=[image_size[0] // 8, image_size[1] // 8], xbound=[-half, half, 0.4],
                            ybound=[-half_y, half_y, 0.4], zbound=[-10.0, 10.0, 20.0], dbound=[1.0, 9.0, 0.5], downsample=2)),
        decoder=dict(backbone=dict(RESNET_CFG), neck=dict(LSSFPN_CFG)),
        bbox_head=bbox_head)


def test_registry_builds_with_the_reference_key_sets():
    from al3d.models import build_backbone, build_detector, build_neck
    resnet = build_backbone(dict(RESNET_CFG))
    assert set(resnet.state_dict()) == RESNET_KEYS
    assert resnet[0][0].conv1.stride == (2, 2) and resnet[2][0].conv1.stride == (1, 1) and resnet[0][1].downsample is None
    fpn = build_neck(dict(LSSFPN_CFG))
    assert set(fpn.state_dict()) == LSSFPN_KEYS and tuple(fpn.state_dict()["fuse.0.weight"].shape) == (256, 640, 1, 1)
    det = build_detector(detector_cfg())
    keys = set(det.state_dict())
    swin = build_backbone(detector_cfg()["camera"]["backbone"])
    cneck = build_neck(detector_cfg()["camera"]["neck"])
    want = {"encoders.camera.backbone." + k for k in swin.state_dict()} | \
        {"encoders.camera.neck." + k for k in cneck.state_dict()} | \
        {"encoders.camera.vtransform." + k for k in LSSTRANSFORM_KEYS} | \
        {"decoder.backbone." + k for k in RESNET_KEYS} | {"decoder.neck." + k for k in LSSFPN_KEYS}
    assert keys == want
    assert det.bbox_head is None and det.prepare({}) is None
    vt = det.encoders["camera"]["vtransform"]
    assert vt.D == 16 and vt.C == 80 and tuple(vt.depthnet.weight.shape) == (96, 256, 1, 1)


def test_golden_state_dicts_load_strictly():
    from al3d.models import build_neck
    z = np.load(GOLD)
    cfg = json.loads(str(z["settings"]))
    assert cfg["dtype"] == "float32"
    fpn = build_neck(dict(cfg["fpn"], type="LSSFPN"))
    fpn.load_state_dict({k[len("fpn.sd."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("fpn.sd.")}, strict=True)
    vt = build_neck(dict(cfg["vtransform"], type="LSSTransform"))
    vt.load_state_dict({k[len("vt.sd."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("vt.sd.")}, strict=True)
    assert vt.D == 5 and vt.C == 8


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def test_yardstick_matches_the_reference_golden():
    """The golden is the reference's float32 output: 1e-5 of the output's largest magnitude."""
    z = np.load(GOLD)
    cfg = json.loads(str(z["settings"]))
    sd = {k[len("fpn.sd."):]: z[k] for k in z.files if k.startswith("fpn.sd.")}
    y = Y.lssfpn64(torch.from_numpy(z["fpn_x1"]), torch.from_numpy(z["fpn_x2"]), sd, cfg["fpn"]["scale_factor"])
    assert tuple(y.shape) == z["fpn_out"].shape and _rel(y.numpy(), z["fpn_out"]) < 1e-5
    sd = {k[len("vt.sd."):]: z[k] for k in z.files if k.startswith("vt.sd.")}
    depth, ctx, prod = Y.cam_feats64(torch.from_numpy(z["vt_x"]), sd, 5, 8)
    assert tuple(prod.shape) == z["vt_cam_feats"].shape and _rel(prod.numpy(), z["vt_cam_feats"]) < 1e-5
    assert torch.allclose(depth.sum(1), torch.ones_like(depth.sum(1)), atol=1e-12)


def test_upsample_yardstick_is_torch_align_corners():
    x = torch.randn(2, 3, 3, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for size in ((6, 10), (7, 9), (3, 5)):
        ref = nn.functional.interpolate(x, size=size, mode="bilinear", align_corners=True)
        assert float((Y.upsample_ac64(x, size) - ref).abs().max()) < 1e-13
    one = torch.randn(1, 4, 1, 1, dtype=torch.float64)
    assert torch.equal(Y.upsample_ac64(one, (2, 2)), one.expand(1, 4, 2, 2))


def nn_block(cin, cout, stride):
    """The standard block from torch.nn pieces (what mmcv's BasicBlock / make_res_layer assemble)."""
    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False)
            self.bn1 = nn.BatchNorm2d(cout)
            self.conv2 = nn.Conv2d(cout, cout, 3, padding=1, bias=False)
            self.bn2 = nn.BatchNorm2d(cout)
            self.downsample = None
            if stride != 1 or cin != cout:
                self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride, bias=False), nn.BatchNorm2d(cout))

        def forward(self, x):
            y = self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x)))))
            return torch.relu(y + (x if self.downsample is None else self.downsample(x)))
    return Block()


def seed_module_(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
            elif name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.75)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        for name, b in m.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) * 0.5 + 0.75)
    return m.eval()


def test_basic_block_yardstick_is_the_torch_nn_block():
    for cin, cout, stride in ((16, 32, 2), (32, 32, 1), (32, 64, 1)):
        blk = seed_module_(nn_block(cin, cout, stride), 7).double()
        x = torch.randn(2, cin, 9, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
        with torch.no_grad():
            ref = blk(x)
        got = Y.basic_block64(x, blk.state_dict(), "", stride)
        assert float((got - ref).abs().max()) < 1e-12
    # and the stage wiring of GeneralizedResNet: this build's module tree holds exactly the yardstick's keys
    from al3d.models import build_backbone
    net = seed_module_(build_backbone(dict(type="GeneralizedResNet", in_channels=16, blocks=[[2, 32, 2], [1, 64, 1]])), 3)
    x = torch.randn(1, 16, 12, 12, generator=torch.Generator().manual_seed(4))
    outs = Y.resnet64(x, net.state_dict(), net.blocks)
    assert [tuple(o.shape) for o in outs] == [(1, 32, 6, 6), (1, 64, 6, 6)]
    ref = x.double()
    for s, (n, c, stride) in enumerate(net.blocks):
        for b in range(n):
            blk = nn_block(ref.shape[1], c, stride if b == 0 else 1).double()
            blk.load_state_dict({k[len(f"{s}.{b}."):]: v.double() for k, v in net.state_dict().items()
                                 if k.startswith(f"{s}.{b}.")}, strict=True)
            with torch.no_grad():
                ref = blk.eval()(ref)
        assert float((outs[s] - ref).abs().max()) < 1e-12
