"""Times the camera-only BEV decoder on one GPU: the fused residual convolution against its two-step form on the decoder's
layer shapes, the decoder as a whole, and the detector per stage.

  python tools/bench_camera_decoder.py [--batch 16] [--grid 128] [--repeats 7] [--out profiles/camera_decoder.txt]

Events around `--iters` back-to-back launches after a warm-up, `--repeats` alternated repeats (fused, two-step, fused, ...);
reported: median and min .. max in microseconds per call."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def alternate(fns, iters, repeats, warmup=5):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            runs[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in runs.items()}


def rig(B, N, image_size):
    """N pinhole cameras looking around the vehicle; identity augmentations."""
    import math
    iH, iW = image_size
    K = torch.eye(4).repeat(B, N, 1, 1)
    K[..., 0, 0] = K[..., 1, 1] = 0.48 * iW
    K[..., 0, 2], K[..., 1, 2] = iW / 2.0, iH / 2.0
    c2l = torch.eye(4).repeat(B, N, 1, 1)
    for n in range(N):
        yaw = 2 * math.pi * n / N + 0.1
        c2l[:, n, :3, :3] = torch.tensor([[math.sin(yaw), 0.0, math.cos(yaw)], [-math.cos(yaw), 0.0, math.sin(yaw)],
                                          [0.0, -1.0, 0.0]])
        c2l[:, n, :3, 3] = torch.tensor([0.5 * math.cos(yaw), 0.5 * math.sin(yaw), 1.5])
    return K, c2l, torch.eye(4).repeat(B, N, 1, 1), torch.eye(4).repeat(B, 1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--detector", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from al3d import detector_ops as D, synthetic
    from al3d.models import build_backbone, build_detector, build_neck
    lines = [f"camera-only BEV decoder, B = {args.batch}, {args.grid} x {args.grid} x 80 in, AL3D_MATH = {D.MATH}; "
             f"us per call: median (min .. max) of {args.repeats} alternated repeats x {args.iters} launches"]
    B, G = args.batch, args.grid
    g = torch.Generator().manual_seed(0)
    for H, C in ((G // 2, 128), (G // 4, 256), (G // 4, 512)):
        x = torch.randn(B, H, H, C, generator=g).to(DEV)
        res = torch.randn(B, H, H, C, generator=g).to(DEV)
        w = (torch.randn(C, 9, C, generator=g) / (9 * C) ** 0.5).to(DEV)
        scale, shift = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        wf, sf = D.pack_res3x3(w, scale)
        wd, sd = D.pack_dense(w, scale, 3, 1, 1)
        fns = {
            "fused": lambda: D.conv3x3_res_nhwc(x, wf, sf, shift, res),
            "two-step (default dispatch)": lambda: D.add_relu_nhwc(D.conv2d_nhwc(x, wd, sd, shift, 3, 1, 1, False), res),
            "two-step (LDS-DMA kernel)": lambda: D.add_relu_nhwc(D.conv2d_nhwc(x, wf, sf, shift, 3, 1, 1, False), res),
        }
        for k, (med, lo, hi) in alternate(fns, args.iters, args.repeats).items():
            lines.append(f"  {B} x {H} x {H} x {C} -> {C}  {k:30s} {med:9.1f} ({lo:.1f} .. {hi:.1f})")
    net = synthetic.seed_modules_(build_backbone(dict(type="GeneralizedResNet", in_channels=80,
                                                      blocks=[[2, 128, 2], [2, 256, 2], [2, 512, 1]])), 1).to(DEV).eval()
    fpn = synthetic.seed_modules_(build_neck(dict(type="LSSFPN", in_indices=[-1, 0], in_channels=[512, 128], out_channels=256,
                                                  scale_factor=2)), 2).to(DEV).eval()
    x = torch.randn(B, G, G, 80, generator=g).to(DEV)
    def decoder(res):
        def run():
            D.RES = res
            return fpn(net(x))
        return run
    default = D.RES
    with torch.no_grad():
        runs = alternate({r: decoder(r) for r in ("fused", "two-step")}, max(args.iters // 4, 2), args.repeats)
    D.RES = default
    for r, (med, lo, hi) in runs.items():
        lines.append(f"  decoder (GeneralizedResNet + LSSFPN), AL3D_RES={r}, {B} x {G} x {G} x 80 -> {2 * (G // 2)}^2 x 256: "
                     f"{med:9.1f} ({lo:.1f} .. {hi:.1f})")
    if args.detector:
        from al3d.utils import Config
        cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_camera_centerhead_entropy.py"))
        det = synthetic.seed_modules_(build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg), 3).to(DEV).eval()
        b = max(B // 8, 1)
        K, c2l, aug, laug = rig(b, 6, (256, 704))
        ex = dict(img=torch.randn(b, 6, 256, 704, 3, generator=g).to(DEV), camera_intrinsics=K.to(DEV), camera2lidar=c2l.to(DEV),
                  img_aug_matrix=aug.to(DEV), lidar_aug_matrix=laug.to(DEV), calib_key="rig")
        stages = []
        with torch.no_grad():
            for i in range(2 + args.repeats):
                det(ex, return_loss=False, estimate=True, timed=True)
                if i >= 2:
                    stages.append(dict(det.stage_ms))
        lines.append(f"  detector per stage, {b} samples x 6 cameras of 256 x 704, ms: median (min .. max) of {args.repeats}")
        for k in stages[0]:
            v = [s[k] for s in stages]
            lines.append(f"    {k:40s} {statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
