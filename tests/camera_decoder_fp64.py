"""Float64 yardstick of the camera-only BEV decoder (BasicBlock, GeneralizedResNet, LSSFPN, LSSTransform.get_cam_feats),
written with plain torch float64 functions on NCHW tensors from state dicts -- no module of the build under test.

LSSFPN and get_cam_feats are pinned to the reference's own output (tests/golden/bevfusion_camera_decoder.npz, which is
FLOAT32: the reference computes in f32, so the pin is 1e-5 relative, not f64 precision); BasicBlock has no reference
source (mmcv's class is not in the reference tree) and is pinned to ``torch.nn`` float64 modules assembled in
tests/test_camera_decoder_cpu.py."""
import torch
import torch.nn.functional as F


def _d(t):
    return torch.as_tensor(t).double()


def bn64(x, sd, p, eps=1e-5):
    """eval BatchNorm2d from state-dict entries ``p + {weight,bias,running_mean,running_var}``."""
    inv = torch.rsqrt(_d(sd[p + "running_var"]) + eps)
    return (x - _d(sd[p + "running_mean"]).view(1, -1, 1, 1)) * (inv * _d(sd[p + "weight"])).view(1, -1, 1, 1) \
        + _d(sd[p + "bias"]).view(1, -1, 1, 1)


def basic_block64(x, sd, p, stride):
    """relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut(x)); shortcut = downsample.{0,1} when the state dict has them."""
    y = F.relu(bn64(F.conv2d(x, _d(sd[p + "conv1.weight"]), stride=stride, padding=1), sd, p + "bn1."))
    y = bn64(F.conv2d(y, _d(sd[p + "conv2.weight"]), padding=1), sd, p + "bn2.")
    idn = x
    if p + "downsample.0.weight" in sd:
        idn = bn64(F.conv2d(x, _d(sd[p + "downsample.0.weight"]), stride=stride), sd, p + "downsample.1.")
    return F.relu(y + idn)


def resnet64(x, sd, blocks, prefix=""):
    """GeneralizedResNet: list of stage outputs; blocks = [(num_blocks, out_channels, stride), ...]."""
    x, outs = _d(x), []
    for s, (n, _, stride) in enumerate(blocks):
        for b in range(n):
            x = basic_block64(x, sd, f"{prefix}{s}.{b}.", stride if b == 0 else 1)
        outs.append(x)
    return outs


def upsample_ac64(x, size):
    """Bilinear, align_corners=True, evaluated from the definition (not through F.interpolate)."""
    x = _d(x)
    h, w = x.shape[-2:]
    H, W = size
    ys = torch.arange(H, dtype=torch.float64) * ((h - 1) / (H - 1) if H > 1 else 0.0)
    xs = torch.arange(W, dtype=torch.float64) * ((w - 1) / (W - 1) if W > 1 else 0.0)
    y0, x0 = ys.floor().long().clamp(max=h - 1), xs.floor().long().clamp(max=w - 1)
    y1, x1 = (y0 + 1).clamp(max=h - 1), (x0 + 1).clamp(max=w - 1)
    ly, lx = (ys - y0).view(-1, 1), (xs - x0).view(1, -1)
    top = x[..., y0, :][..., x0] * (1 - lx) + x[..., y0, :][..., x1] * lx
    bot = x[..., y1, :][..., x0] * (1 - lx) + x[..., y1, :][..., x1] * lx
    return top * (1 - ly) + bot * ly


def lssfpn64(x1, x2, sd, scale_factor, prefix=""):
    """necks/lss.py:47-65 with x1 = x[in_indices[0]], x2 = x[in_indices[1]]."""
    x = torch.cat([upsample_ac64(x1, x2.shape[-2:]), _d(x2)], dim=1)
    x = F.relu(bn64(F.conv2d(x, _d(sd[prefix + "fuse.0.weight"])), sd, prefix + "fuse.1."))
    x = F.relu(bn64(F.conv2d(x, _d(sd[prefix + "fuse.3.weight"]), padding=1), sd, prefix + "fuse.4."))
    if scale_factor > 1:
        x = upsample_ac64(x, (x.shape[-2] * scale_factor, x.shape[-1] * scale_factor))
        x = F.relu(bn64(F.conv2d(x, _d(sd[prefix + "upsample.1.weight"]), padding=1), sd, prefix + "upsample.2."))
    return x


def cam_feats64(x, sd, D, C, prefix=""):
    """vtransforms/lss.py:61-73: x [B,N,Cin,fH,fW] -> (depth [BN,D,fH,fW], context [BN,C,fH,fW], their product
    [B,N,D,fH,fW,C] -- the reference's return value)."""
    B, N, Cin, fH, fW = x.shape
    y = F.conv2d(_d(x).view(B * N, Cin, fH, fW), _d(sd[prefix + "depthnet.weight"]), _d(sd[prefix + "depthnet.bias"]))
    depth, ctx = y[:, :D].softmax(dim=1), y[:, D:D + C]
    prod = (depth.unsqueeze(1) * ctx.unsqueeze(2)).view(B, N, C, D, fH, fW).permute(0, 1, 3, 4, 5, 2)
    return depth, ctx, prod


def abs_state(sd, eps=1e-5):
    """State dict of the ABS CHAIN of a module: conv weights and biases by magnitude, every BatchNorm replaced by
    |scale|, |shift| of its folded form.  The yardstick functions above, run on |x| with this state dict, give per output
    element the normaliser of tests/dense_fp64.py carried through the module: the sum of |a*b| of every layer with the
    magnitudes of the layers before it as input (ReLU and the bilinear blend, whose weights are positive, pass it on).
    A split-arithmetic layer errs by at most dense_fp64.E_MAX of its own normaliser, an earlier layer's error reaches the
    output through at most the later layers' abs chain, so L layers in sequence err by at most L * E_MAX * this."""
    out = {}
    for k, v in sd.items():
        v = torch.as_tensor(v).double()
        out[k] = v.abs() if (v.dim() > 1 or k.endswith("depthnet.bias")) else v
    for k in sd:
        if k.endswith("running_var"):
            p = k[:-len("running_var")]
            inv = torch.rsqrt(_d(sd[p + "running_var"]) + eps) * _d(sd[p + "weight"])
            shift = _d(sd[p + "bias"]) - _d(sd[p + "running_mean"]) * inv
            out[p + "weight"], out[p + "bias"] = inv.abs(), shift.abs()
            out[p + "running_mean"], out[p + "running_var"] = torch.zeros_like(inv), torch.ones_like(inv) - eps
    return out
