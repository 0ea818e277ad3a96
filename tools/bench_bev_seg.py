"""Times the BEV map segmentation head on one GPU at the workload's shapes: the grid resample and the classifier kernel per
launch, and the whole head, each beside the same step built from torch's library ops on the same card, alternated in one
process (``F.grid_sample`` + ``nn.Conv2d`` + ``torch.sigmoid`` on channels-last tensors: the reference's own code path).

  python tools/bench_bev_seg.py [--batch 16] [--classes 6] [--iters 10] [--repeats 7] [--out profiles/bev_seg.txt]

Events around ``--iters`` back-to-back launches after a warm-up, ``--repeats`` alternated repeats; reported: median and
min .. max in microseconds per call, and for the two new kernels the bytes they must move (source read once + output
written once; the classifier: map in, probabilities out) over the median time, as a fraction of the 6.3 TB/s a streaming
kernel achieves on this part (8 TB/s is the HBM3E peak).  ``al3d_upsample_bilinear_ac_nhwc_f32`` is timed on the same
byte count as the resample for comparison."""
import argparse
import copy
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_camera_decoder import alternate  # noqa: E402

DEV = "cuda:0"
HBM_ACHIEVABLE = 6.3e12
# (source cells, channels, input scope): the camera / fusion decoders' 128 x 128 x 256 map of 0.8 m cells, the lidar
# decoder's 180 x 180 x 512 map of 0.6 m cells; output: the map grid of configs/nuscenes/seg/default.yaml
SHAPES = [(128, 256, (-51.2, 51.2, 0.8)), (180, 512, (-54.0, 54.0, 0.6))]
OUT_SCOPE = (-50.0, 50.0, 0.5)


def torch_grid(B, in_scope, device):
    v = torch.arange(OUT_SCOPE[0] + OUT_SCOPE[2] / 2, OUT_SCOPE[1], OUT_SCOPE[2])
    v = ((v - in_scope[0]) / (in_scope[1] - in_scope[0]) * 2 - 1).to(device)
    u, w = torch.meshgrid([v, v], indexing="ij")
    return torch.stack([torch.stack([w, u], dim=-1)] * B, dim=0)


def fmt(name, stat, bytes_moved=None):
    med, lo, hi = stat
    line = f"  {name:58s} {med:10.1f} ({lo:.1f} .. {hi:.1f})"
    if bytes_moved is not None:
        rate = bytes_moved / (med * 1e-6)
        line += f"   {bytes_moved / 1e6:8.1f} MB  {rate / 1e12:5.2f} TB/s = {100.0 * rate / HBM_ACHIEVABLE:5.1f} % of 6.3 TB/s"
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--head", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from al3d import detector_ops as D, synthetic
    from al3d.models import build_head
    B, K = args.batch, args.classes
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    emit(f"BEV map segmentation head, B = {B}, K = {K}, output grid 200 x 200, AL3D_MATH = {D.MATH}; us per call: median "
         f"(min .. max) of {args.repeats} alternated repeats x {args.iters} launches; 'torch': the same step from torch's "
         "library ops (channels-last) in the same process")
    g = torch.Generator().manual_seed(0)
    for S, C, in_scope in SHAPES:
        i_s, o_s = [in_scope, in_scope], [OUT_SCOPE, OUT_SCOPE]
        x = torch.randn(B, S, S, C, generator=g).to(DEV)
        x_nchw = x.permute(0, 3, 1, 2)                                  # channels-last NCHW view for torch
        grid = torch_grid(B, in_scope, DEV)
        y = D.bev_grid_resample_nhwc(x, i_s, o_s)
        H, W = y.shape[1:3]
        assert (H, W) == (200, 200) and float((y.permute(0, 3, 1, 2) - F.grid_sample(x_nchw, grid, mode="bilinear", align_corners=False)).abs().max()) < 1e-3
        moved = 4 * (x.numel() + y.numel())
        emit(f"{B} x {S} x {S} x {C} -> 200 x 200")
        stats = alternate({"al3d_bev_grid_resample_nhwc_f32": lambda: D.bev_grid_resample_nhwc(x, i_s, o_s),
                           "al3d_bev_grid_resample_nhwc_f32, out_hw_swapped": lambda: D.bev_grid_resample_nhwc(x, i_s, o_s, True),
                           "al3d_upsample_bilinear_ac_nhwc_f32 (same bytes)": lambda: D.upsample_bilinear_ac_nhwc(x, (H, W)),
                           "torch F.grid_sample": lambda: F.grid_sample(x_nchw, grid, mode="bilinear", align_corners=False)},
                          args.iters, args.repeats)
        for k, s in stats.items():
            emit(fmt(k, s, None if k.startswith("torch") else moved))
        conv = torch.nn.Conv2d(C, K, 1).to(DEV).to(memory_format=torch.channels_last).eval()
        w, b = conv.weight.detach().reshape(K, C).contiguous(), conv.bias.detach()
        y_nchw = y.permute(0, 3, 1, 2)
        with torch.no_grad():
            assert float((D.seg_classify(y, w, b) - torch.sigmoid(conv(y_nchw))).abs().max()) < 1e-3
            stats = alternate({"al3d_seg_classify_f32 (probabilities)": lambda: D.seg_classify(y, w, b),
                               "al3d_seg_classify_f32 (+ entropy, area)": lambda: D.seg_classify(y, w, b, with_stats=True),
                               "torch Conv2d(C, K, 1) + sigmoid": lambda: torch.sigmoid(conv(y_nchw))}, args.iters, args.repeats)
        moved = 4 * (y.numel() + B * K * H * W)
        for k, s in stats.items():
            emit(fmt(k, s, None if k.startswith("torch") else moved))
        if not args.head:
            continue
        classes = [f"class{i}" for i in range(K)]
        head = synthetic.seed_modules_(build_head(dict(type="BEVSegmentationHead", in_channels=C, classes=classes, loss="focal",
                                                       grid_transform=dict(input_scope=i_s, output_scope=o_s))), 5).to(DEV).eval()
        ref = copy.deepcopy(head.classifier)                           # plain torch.nn modules with the same parameters
        ref = ref.to(DEV).to(memory_format=torch.channels_last).eval()

        def torch_head():
            return torch.sigmoid(ref(F.grid_sample(x_nchw, grid, mode="bilinear", align_corners=False)))
        with torch.no_grad():
            d = float((head(x) - torch_head()).abs().max())
            assert d < 1e-3, d
            stats = alternate({"head (al3d, with entropy and area)": lambda: head(x, with_stats=True), "head (torch)": torch_head},
                              max(args.iters // 5, 2), args.repeats, warmup=2)
        for k, s in stats.items():
            emit(fmt(k, s))
        del head, ref
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
