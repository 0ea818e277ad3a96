"""GPU suite of the camera-only BEV decoder: the fused residual convolution (csrc/conv2d_res.hip) against its two-step form
(bit for bit) and the float64 yardstick, the bilinear upsample, the argument contract, the modules against the reference
golden, and the registered detector end to end.

Measured on one MI355X, maximum absolute error against float64 (existing convolution without residual / fused launch
with residual and ReLU; outputs up to 10-15 in magnitude): 2x5x7 16->32: 9.36e-07 / 9.36e-07; 1x16x16 128->128: 4.04e-06 /
3.81e-06; 1x8x8 512->512: 7.33e-06 / 6.70e-06; 8x62x63 16->128 (two channel tiles per wave): 2.01e-06 / 2.02e-06.  One
BasicBlock under bf16x6 / f32: 8.1e-09 / 8.6e-09 of the abs-chain normaliser.  Also in DESIGN 8d."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import camera_decoder_fp64 as Y
from test_camera_decoder_cpu import GOLD, detector_cfg, seed_module_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 5, 7, 16, 32), (1, 16, 16, 128, 128), (1, 8, 8, 512, 512)]      # B, H, W, Cin, Cout
# 8 x 16 x 8 pixel tiles x 4 channel tiles = 4,096 wave tiles: the launch takes two channel tiles per wave (the decoder's own
# layers at B = 16 all do); 62 x 63: tile remainders in both axes on that path too
WIDE = [(8, 62, 63, 16, 128)]
_CASES = {}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def case(shape):
    """Inputs of one layer, its f16x3 weights, and the float64 reference of the plain convolution -- built once."""
    if shape not in _CASES:
        from al3d import detector_ops as D
        B, H, W, cin, cout = shape
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randn(B, cin, H, W, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        scale = (torch.rand(cout, generator=g) * 0.5 + 0.75) * torch.where(torch.rand(cout, generator=g) < 0.25, -1.0, 1.0)
        shift = torch.randn(cout, generator=g) * 0.5 - 0.5                  # pre-activations of both signs
        res = torch.randn(B, cout, H, W, generator=g) * 3.0                 # large enough to flip the sign
        ref = torch.nn.functional.conv2d(x.double(), w.double(), padding=1) * scale.double().view(1, -1, 1, 1) \
            + shift.double().view(1, -1, 1, 1)
        wp, sc = D.dense_pack("dma", D.pack_conv_weight(w).to(DEV), scale.to(DEV))
        _CASES[shape] = dict(x=nhwc(x).to(DEV), res=nhwc(res).to(DEV), shift=shift.to(DEV), wp=wp, sc=sc, ref=nhwc(ref),
                             res64=nhwc(res).double(), w=w, scale=scale)
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES + WIDE)
@pytest.mark.parametrize("relu", [True, False])
def test_fused_equals_two_step_exactly(shape, relu):
    from al3d import detector_ops as D
    assert D.MATH == "f16x3"
    c = case(shape)
    B, H, W, cin, cout = shape
    two = D.add_relu_nhwc(D.conv2d_nhwc(c["x"], c["wp"], c["sc"], c["shift"], 3, 1, 1, False), c["res"], relu)
    got = D.conv3x3_res_nhwc(c["x"], c["wp"], c["sc"], c["shift"], c["res"], relu=relu)
    assert got.shape == (B, H, W, cout) and torch.equal(got, two)
    if relu:
        pre = c["ref"] + c["res64"]
        assert bool((got == 0).any()) and bool((got > 0).any()) and bool(((c["ref"] < 0) & (pre > 0)).any())
    # a residual wider than the output (ldr != C), written into a window of a wider map (coff, ldc)
    wide = torch.cat([c["res"], torch.full((B, H, W, 8), 7.0, device=DEV)], dim=-1).contiguous()
    out = torch.full((B, H, W, cout + 12), -5.0, device=DEV)
    D.conv3x3_res_nhwc(c["x"], c["wp"], c["sc"], c["shift"], wide, relu=relu, out=out, coff=8)
    assert torch.equal(out[..., 8:8 + cout], two)
    assert bool((out[..., :8] == -5.0).all()) and bool((out[..., 8 + cout:] == -5.0).all())


@pytest.mark.parametrize("shape", SHAPES + WIDE)
def test_fused_within_twice_the_parent_convs_error(shape):
    """Bound: twice the existing f16x3 3x3 convolution's own measured error on the layer without residual (the kernels of the
    parent commit: the default dispatch and the LDS-DMA kernel, whichever is larger) -- the residual path adds one rounding
    and the yardstick is exact -- plus one f32 ulp of |res| for the add."""
    from al3d import detector_ops as D
    c = case(shape)
    wd, sd = D.pack_dense(D.pack_conv_weight(c["w"]).to(DEV), c["scale"].to(DEV), 3, 1, 1)
    e_parent = 0.0
    for w, s in ((wd, sd), (c["wp"], c["sc"])):
        plain = D.conv2d_nhwc(c["x"], w, s, c["shift"], 3, 1, 1, False)
        e_parent = max(e_parent, float((plain.cpu().double() - c["ref"]).abs().max()))
    got = D.conv3x3_res_nhwc(c["x"], c["wp"], c["sc"], c["shift"], c["res"], relu=True).cpu().double()
    ref = torch.relu(c["ref"] + c["res64"])
    ulp = torch.from_numpy(np.spacing(np.abs(c["res64"].numpy().astype(np.float32)))).double()
    diff = (got - ref).abs()
    print(f"shape {shape}: parent conv max err {e_parent:.3e}, fused max err {float(diff.max()):.3e}, "
          f"max |ref| {float(ref.abs().max()):.3f}")
    assert e_parent > 0 and bool((diff <= 2.0 * e_parent + ulp).all())


def test_other_arithmetics_in_a_child_process():
    """One BasicBlock with a downsample shortcut under bf16x6 and f32 at the bound of test_dense_gpu.py: dense_fp64.E_MAX of
    the abs-chain normaliser (camera_decoder_fp64.abs_state).  The child also writes a channel window of a wider map
    through the two-step path and must refuse a window that does not fit."""
    from dense_fp64 import E_MAX
    for math in ("bf16x6", "f32"):
        env = dict(os.environ, AL3D_MATH=math)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "camera_decoder_worker.py")], env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        print(out)
        assert out["math"] == math and out["finite"] and out["shape"] == [2, 64, 4, 4] and out["err"] < E_MAX
        assert out["window"] and out["refused"]


@pytest.mark.parametrize("sizes", [((3, 5), (6, 10)), ((1, 1), (2, 2))])
def test_upsample_equals_the_cat_kernels_align_corners_branch(sizes):
    from al3d import detector_ops as D, lib
    from al3d.selector_ops import _ptr, _stream
    (h, w), (H, W) = sizes
    g = torch.Generator().manual_seed(9)
    src = torch.randn(2, 8, h, w, generator=g)
    lat = torch.randn(2, H, W, 4, generator=g).to(DEV)
    s = nhwc(src).to(DEV)
    cat = torch.empty((2, H, W, 12), device=DEV)
    lib.call("al3d_lss_upsample_cat_mode_f32", _ptr(lat), _ptr(s), 2, H, W, 4, h, w, 8, 1, _ptr(cat), _stream())
    got = D.upsample_bilinear_ac_nhwc(s, (H, W))
    assert torch.equal(got, cat[..., 4:])
    ref = nhwc(Y.upsample_ac64(src, (H, W)))
    assert float((got.cpu().double() - ref).abs().max()) < 1e-6


def test_argument_contract():
    from al3d import detector_ops as D, lib
    from al3d.selector_ops import _ptr, _stream

    def call(x, wgt, scale, res, out, cin, cout, ldr):
        B, H, W = x.shape[:3]
        lib.call("al3d_conv3x3_res_nhwc_f16x3", _ptr(x), _ptr(wgt), _ptr(scale), None, _ptr(res), _ptr(out), B, H, W, cin, cout,
                 ldr, out.shape[3], 0, 1, _stream())
    x = torch.randn(1, 4, 4, 32, device=DEV)
    wgt = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    scale = torch.ones(64, device=DEV)
    res = torch.randn(1, 4, 4, 64, device=DEV)
    for cin, cout, r, ldr, word in ((32, 48, res, 64, "Cout=48"), (24, 32, res, 64, "Cin=24"), (32, 32, None, 64, "null residual"),
                                    (32, 64, res, 32, "ldr=32")):
        out = torch.full((1, 4, 4, 64), -3.0, device=DEV)
        with pytest.raises(lib.Al3dError, match=word):
            call(x, wgt, scale, r, out, cin, cout, ldr)
        torch.cuda.synchronize()
        assert bool((out == -3.0).all())
    # the Python entry: weights of another structure are an error, not a detour
    w = torch.randn(128, 9, 32, device=DEV)
    wp, sc = D.dense_pack("frag3x3", w, None)
    with pytest.raises(lib.Al3dError):
        D.conv3x3_res_nhwc(x, wp, sc, None, torch.randn(1, 4, 4, 128, device=DEV))


def _bound(got, ref64, norm64, layers, what):
    """Elementwise: |got - ref| <= layers * E_MAX * norm, norm = the module's abs chain on |input|
    (camera_decoder_fp64.abs_state: E_MAX of its own normaliser per layer, carried to the output by the layers after it)."""
    from dense_fp64 import E_MAX
    e = ((got.cpu().double() - ref64).abs() / norm64).max()
    print(f"{what}: {float(e):.3e} of the abs-chain normaliser (bound {layers} x {E_MAX:.1e})")
    assert float(e) <= layers * E_MAX, (what, float(e))


def _golden(got, gold, what):
    """Against the reference's float32 output: 1e-5 of its largest magnitude, the pin of the yardstick itself."""
    gold = gold.double()
    e = float((got.cpu().double() - gold).abs().max() / gold.abs().max())
    print(f"{what}: {e:.3e} of the largest magnitude")
    assert e < 1e-5, (what, e)


def test_modules_against_the_reference_golden():
    from al3d.models import build_neck
    z = np.load(GOLD)
    cfg = json.loads(str(z["settings"]))
    sd = {k[len("fpn.sd."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("fpn.sd.")}
    fpn = build_neck(dict(cfg["fpn"], type="LSSFPN"))
    fpn.load_state_dict(sd, strict=True)
    fpn = fpn.to(DEV).eval()
    x1, x2 = torch.from_numpy(z["fpn_x1"]), torch.from_numpy(z["fpn_x2"])
    with torch.no_grad():
        y = fpn([nhwc(x2).to(DEV), nhwc(x1).to(DEV)])
    ref = Y.lssfpn64(x1, x2, sd, 2)
    norm = Y.lssfpn64(x1.abs(), x2.abs(), Y.abs_state(sd), 2)
    # five steps in sequence: resize (three f32 blends, < E_MAX of their magnitudes), 1x1, 3x3, resize, 3x3
    _bound(y, nhwc(ref), nhwc(norm), 5, "LSSFPN vs yardstick")
    _golden(y, nhwc(torch.from_numpy(z["fpn_out"])), "LSSFPN vs golden")
    sd = {k[len("vt.sd."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("vt.sd.")}
    vt = build_neck(dict(cfg["vtransform"], type="LSSTransform"))
    vt.load_state_dict(sd, strict=True)
    vt = vt.to(DEV).eval()
    x = torch.from_numpy(z["vt_x"])
    with torch.no_grad():
        depth, ctx = vt.get_cam_feats(x.permute(0, 1, 3, 4, 2).contiguous().to(DEV))
    d64, c64, _ = Y.cam_feats64(x, sd, 5, 8)
    w, b = sd["depthnet.weight"].double(), sd["depthnet.bias"].double()
    logits = torch.nn.functional.conv2d(x.double().view(2, 16, 4, 6), w, b)
    lnorm = torch.nn.functional.conv2d(x.double().abs().view(2, 16, 4, 6), w.abs(), b.abs())
    _bound(ctx, nhwc(c64), nhwc(lnorm[:, 5:13]), 1, "context vs yardstick")
    # softmax over D = 5 logits, each off by at most e_l = E_MAX * (largest logit normaliser of the pixel): the shifted
    # argument errs by 2 e_l + one rounding of |arg|, expf adds <= 2 ulp, the sum of D terms and the division one each;
    # a probability's relative error is at most twice the largest term error plus those
    from dense_fp64 import E_MAX
    u = 2.0 ** -24
    e_l = E_MAX * lnorm[:, :5].amax(1, keepdim=True)
    arg = (logits[:, :5] - logits[:, :5].amax(1, keepdim=True)).abs().amax(1, keepdim=True)
    rel = 2.0 * (2.0 * e_l + u * arg + 2.0 * u) + (5 + 1) * u
    derr = (depth.cpu().double() - d64).abs()
    print(f"depth probabilities: max err {float(derr.max()):.3e}, max of err / bound {float((derr / (rel * d64)).max()):.3f}")
    assert bool((derr <= rel * d64).all())
    prod = depth.view(1, 2, 5, 4, 6, 1) * ctx.view(1, 2, 1, 4, 6, 8)
    _golden(prod, torch.from_numpy(z["vt_cam_feats"]), "depth x context vs golden")


@pytest.mark.parametrize("res", ["fused", "two-step"])
def test_generalized_resnet_against_the_yardstick(res, monkeypatch):
    from al3d import detector_ops as D
    from al3d.models import build_backbone
    monkeypatch.setattr(D, "RES", res)
    net = seed_module_(build_backbone(dict(type="GeneralizedResNet", in_channels=16, blocks=[[2, 32, 2], [1, 64, 1]])), 3)
    x = torch.randn(1, 16, 12, 12, generator=torch.Generator().manual_seed(4))
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    refs = Y.resnet64(x, sd, net.blocks)
    norms = Y.resnet64(x.abs(), Y.abs_state(sd), net.blocks)
    with torch.no_grad():
        outs = net.to(DEV).eval()(nhwc(x).to(DEV))
    assert [tuple(o.shape) for o in outs] == [(1, 6, 6, 32), (1, 6, 6, 64)]
    for i, (o, r, n) in enumerate(zip(outs, refs, norms)):
        _bound(o, nhwc(r), nhwc(n), 2 * sum(b[0] for b in net.blocks[:i + 1]), f"GeneralizedResNet stage {i} ({res})")


def _rig(B, N, image_size):
    iH, iW = image_size
    K = torch.eye(4).repeat(B, N, 1, 1)
    K[..., 0, 0] = K[..., 1, 1] = 0.48 * iW
    K[..., 0, 2], K[..., 1, 2] = iW / 2.0, iH / 2.0
    c2l = torch.eye(4).repeat(B, N, 1, 1)
    for n in range(N):
        yaw = 2 * np.pi * n / N + 0.1
        fwd = torch.tensor([np.cos(yaw), np.sin(yaw), 0.0])
        right = torch.tensor([np.sin(yaw), -np.cos(yaw), 0.0])
        down = torch.tensor([0.0, 0.0, -1.0])
        c2l[:, n, :3, :3] = torch.stack([right, down, fwd], 1).float()
        c2l[:, n, :3, 3] = torch.tensor([0.5 * np.cos(yaw), 0.5 * np.sin(yaw), 1.5]).float()
    return K, c2l, torch.eye(4).repeat(B, N, 1, 1), torch.eye(4).repeat(B, 1, 1)


def test_detector_end_to_end_and_bevfusion_unchanged():
    from al3d import synthetic
    from al3d.datasets import CameraLidarSweepLoader, PoolFrames
    from al3d.models import build_detector
    from al3d.utils import Config
    # the camera+lidar detector on its own smallest input, before anything of the camera-only one has run
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_camera_lidar_spatial_temporal_feature.py"))
    fusion = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(fusion.lidar, seed=0)
    for i, m in enumerate((fusion.camera_backbone, fusion.camera_neck, fusion.vtransform, fusion.fuser)):
        synthetic.seed_modules_(m, 60 + i)
    fusion = fusion.to(DEV).eval()
    pool = PoolFrames.from_synthetic(1, DEV, num_base=1, seed=11)
    ex_f = next(iter(CameraLidarSweepLoader(pool, cfg.voxel_generator, None, 1, device=DEV, num_image_base=1, seed=5)))
    with torch.no_grad():
        before = fusion(ex_f, return_loss=False, estimate=True)[1][-1].mean(-1).mean(-1).clone()

    head = dict(type="CenterHead", in_channels=256, share_conv_channel=64, norm_bbox=True, transpose_input=False,
                tasks=[["car"], ["truck", "bus"]],
                common_heads=dict(reg=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2], vel=[2, 2]),
                separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3),
                test_cfg=dict(post_center_limit_range=[-8.0, -8.0, -10.0, 8.0, 8.0, 10.0], max_pool_nms=False,
                              min_radius=[4, 12], score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1],
                              nms_type=["circle", "rotate"], nms_scale=[[1.0], [1.0, 1.0]], pre_max_size=100, post_max_size=20,
                              nms_thr=0.2),
                bbox_coder=dict(type="CenterPointBBoxCoder", pc_range=[-6.4, -3.2],
                                post_center_range=[-8.0, -8.0, -10.0, 8.0, 8.0, 10.0], max_num=50, score_threshold=0.1,
                                out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9))
    det = build_detector(detector_cfg((64, 96), 32, head, grid_y=16))      # 16 x 8 cells out: x and y cannot be confused
    synthetic.seed_modules_(det, 70)
    det = det.to(DEV).eval()
    B, N = 1, 2
    K, c2l, img_aug, lidar_aug = _rig(B, N, (64, 96))
    ex = dict(img=torch.randn(B, N, 64, 96, 3, generator=torch.Generator().manual_seed(12)).to(DEV),
              camera_intrinsics=K.to(DEV), camera2lidar=c2l.to(DEV), img_aug_matrix=img_aug.to(DEV),
              lidar_aug_matrix=lidar_aug.to(DEV), metadata=[dict(index=0)])
    with torch.no_grad():
        out, middle = det(ex, return_loss=False, estimate=True)
    emb = middle[-1].mean(-1).mean(-1)
    assert tuple(middle[-1].shape) == (1, 256, 16, 8) and tuple(emb.shape) == (1, 256) and bool(torch.isfinite(emb).all())
    assert float(emb.abs().max()) > 0 and len(out) == 1 and out[0]["metadata"]["index"] == 0
    assert det.prepare(ex) is None
    with pytest.raises(NotImplementedError):
        det(ex, return_loss=True)
    with pytest.raises(KeyError):
        det({k: v for k, v in ex.items() if k != "img"}, return_loss=False, estimate=True)
    # orientation: the BEV grid is 16 (x) by 8 (y) cells, the decoder map and the head's buffer keep [x, y] (shapes above and
    # below), and a peak at cell (x = 11, y = 3) of task 0's heat map decodes to that cell's metric centre.  The heads' last
    # layers are silenced (zero weights; biases 0, reg 0.5 = the cell centre, heat maps -10), then the peak is planted in the head's output buffer.
    head_m = det.bbox_head
    with torch.no_grad():
        for th in head_m.task_heads:
            for name in th.heads:
                last = getattr(th, name)[-1]
                last.weight.zero_()
                last.bias.fill_({"heatmap": -10.0, "reg": 0.5}.get(name, 0.0))
        dec = middle[-1].nhwc
        preds = head_m(dec)
        _, spans = head_m._layout()
        assert tuple(preds.fused.shape[:3]) == (1, 16, 8)
        preds.fused[0, 11, 3, spans[0]["heatmap"][0]] = 5.0
        boxes = head_m.get_bboxes(preds)
    assert len(boxes) == 1 and boxes[0]["bboxes"].shape == (1, 9) and int(boxes[0]["labels"][0]) == 0
    cx, cy = float(boxes[0]["bboxes"][0, 0]), float(boxes[0]["bboxes"][0, 1])
    assert abs(cx - ((11 + 0.5) * 0.8 - 6.4)) < 1e-5 and abs(cy - ((3 + 0.5) * 0.8 - 3.2)) < 1e-5
    with torch.no_grad():
        after = fusion(ex_f, return_loss=False, estimate=True)[1][-1].mean(-1).mean(-1)
    assert torch.equal(before, after)
