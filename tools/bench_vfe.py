"""Dev tool: the fused VFE reader (al3d_vfe_net_f32, csrc/vfe.hip) against a torch restatement of the same module on
the same device, at the workload's own shape: M = 2 x 60,000 voxels, T = 10 slots, F = 5 features, num_filters [32, 128].

* ``fused_us``: one ``VoxelFeatureExtractor.forward`` (one launch), device events around ``calls`` calls after ``warmup``
  warm-up calls; ``torch_us``: the reference's op sequence (voxel_encoder.py:13-108: linear, BatchNorm1d in eval mode
  between two permute copies, relu, max, repeat, cat, mask) with library ops on the same tensors.  Three windows each,
  alternating, the median reported; the windows are listed.
* ``module_gflop``: 2 * (K1*U1 + 2*U1*U2 + C*C) per slot over all M * T slots -- what the module as written computes;
  ``kernel_gflop``: the same per row over the rows the kernel computes (the real slots, one padded representative in
  vfe1).  ``gflops`` = kernel_gflop / fused time; ``share_of_fp32_vector_peak`` = that over 157.3 TFLOP/s (the fp32 vector
  peak of the MI355X).  The bytes (M*T*F*4 in, M*C*4 out) at 8 TB/s are ``hbm_floor_us``: the kernel is compute-bound.
* ``max_abs_diff``: fused against the torch restatement on the timed inputs (both f32).

Counts are uniform in 1..T (seeded); ``--full`` fills every slot.  The per-kernel time comes from a run of its own under
``rocprofv3 --kernel-trace --stats`` (kernel vfe_net_kernel).

  python tools/bench_vfe.py [--frames 2] [--voxels 60000] [--calls 20] [--warmup 5] [--full]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch.nn import functional as Fn  # noqa: E402

from al3d import synthetic  # noqa: E402
from al3d.models import build_reader  # noqa: E402

PEAK_FP32_VECTOR = 157.3e12
HBM_BYTES_PER_S = 8.0e12


def torch_vfe(mod, features, num_voxels):
    """The reference forward, op for op, on the module's own parameters (eval mode)."""
    def vfe(layer, x):
        t = x.shape[1]
        x = layer.linear(x)
        x = layer.norm(x.permute(0, 2, 1).contiguous()).permute(0, 2, 1).contiguous()
        pointwise = Fn.relu(x)
        agg = pointwise.max(dim=1, keepdim=True)[0]
        return torch.cat([pointwise, agg.repeat(1, t, 1)], dim=2)

    mean = features[:, :, :3].sum(dim=1, keepdim=True) / num_voxels.type_as(features).view(-1, 1, 1)
    x = torch.cat([features, features[:, :, :3] - mean], dim=-1)
    mask = (torch.arange(features.shape[1], device=features.device)[None, :] < num_voxels[:, None]).unsqueeze(-1)
    mask = mask.type_as(features)
    x = vfe(mod.vfe1, x) * mask
    x = vfe(mod.vfe2, x) * mask
    x = mod.linear(x)
    x = mod.norm(x.permute(0, 2, 1).contiguous()).permute(0, 2, 1).contiguous()
    x = Fn.relu(x) * mask
    return x.max(dim=1)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--voxels", type=int, default=60000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    M, T, F, filters = a.frames * a.voxels, 10, 5, [32, 128]
    mod = build_reader(dict(type="VoxelFeatureExtractor", num_input_features=F, num_filters=filters))
    synthetic.seeded_init_(mod, seed=0)
    mod = mod.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    num = (torch.full((M,), T) if a.full else torch.randint(1, T + 1, (M,), generator=g)).to(torch.int32)
    vox = torch.rand((M, T, F), generator=g)
    vox[:, :, :3] = vox[:, :, :3] * 0.1 + torch.tensor([-40.0, 30.0, -2.0]) + torch.rand((M, 1, 3), generator=g) * 16 - 8
    vox = (vox * (torch.arange(T)[None, :] < num[:, None]).unsqueeze(-1)).to(dev)
    num = num.to(dev)

    def window(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.calls * 1000.0

    with torch.no_grad():
        got, ref = mod(vox, num), torch_vfe(mod, vox, num)
        diff = float((got - ref).abs().max())
        fused, lib_ = [], []
        for _ in range(3):
            fused.append(window(lambda: mod(vox, num)))
            lib_.append(window(lambda: torch_vfe(mod, vox, num)))
    k1, u1, u2, c = F + 3, filters[0] // 2, filters[1] // 2, filters[1]
    n = num.to(torch.int64).clamp(0, T)
    rows12 = int((n + (n < T)).sum())
    rows3 = int(n.sum())
    module_flop = 2.0 * (k1 * u1 + 2 * u1 * u2 + c * c) * M * T
    kernel_flop = 2.0 * (k1 * u1 * rows12 + 2 * u1 * u2 * rows3 + c * c * rows3)
    t_f, t_t = sorted(fused)[1], sorted(lib_)[1]
    hbm = (M * T * F * 4 + M * c * 4) / HBM_BYTES_PER_S * 1e6
    print(json.dumps(dict(
        M=M, T=T, F=F, num_filters=filters, real_slots=rows3, fused_us=round(t_f, 1),
        fused_us_windows=[round(t, 1) for t in fused], torch_us=round(t_t, 1),
        torch_us_windows=[round(t, 1) for t in lib_], speedup=round(t_t / t_f, 2),
        module_gflop=round(module_flop / 1e9, 2), kernel_gflop=round(kernel_flop / 1e9, 2),
        gflops=round(kernel_flop / t_f / 1e3, 1), share_of_fp32_vector_peak=round(kernel_flop / (t_f * 1e-6) / PEAK_FP32_VECTOR, 4),
        hbm_floor_us=round(hbm, 1), compute_floor_us=round(kernel_flop / PEAK_FP32_VECTOR * 1e6, 1), bound="compute",
        max_abs_diff=diff, out_abs_max=float(ref.abs().max()))))


if __name__ == "__main__":
    main()
