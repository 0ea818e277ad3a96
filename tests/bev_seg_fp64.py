"""Float64 yardstick of the BEV map segmentation head (``BEVGridTransform`` + ``BEVSegmentationHead``, reference
bevfusion/mmdet3d/models/heads/segm/vanilla.py:47-138), written with plain torch float64 on NCHW tensors from state dicts
-- no module of the build under test.  The grid resample is evaluated from its definition (the bilinear sample with zero
padding, align_corners=False), not through ``F.grid_sample``; tests/test_bev_seg_cpu.py pins it to torch's CPU
``F.grid_sample`` and the whole head to the reference's own output (tests/golden/bev_seg_head.npz, which is FLOAT32: the
reference computes in f32, so that pin is 1e-5 relative, as tests/camera_decoder_fp64.py explains)."""
import math

import torch
import torch.nn.functional as F

from camera_decoder_fp64 import _d, abs_state, bn64   # noqa: F401  (abs_state: the abs-chain normaliser's state dict)

U = 2.0 ** -24                                        # unit roundoff of float32


def out_size(omin, omax, ostep):
    """Length of ``torch.arange(omin + ostep / 2, omax, ostep)``: ceil((end - start) / step) in double (ATen)."""
    return max(0, int(math.ceil((float(omax) - (float(omin) + float(ostep) / 2)) / float(ostep))))


def axis64(in_scope, out_scope, size):
    """One axis: (i0 [n] int64, w0 [n], w1 [n]) -- the lower neighbour ``floor(pos)`` of every output coordinate and the
    weights of it and of ``i0 + 1``, before padding.  pos = ((g + 1) * size - 1) / 2, g = (v - imin) / (imax - imin) * 2 - 1,
    v = omin + ostep / 2 + k * ostep."""
    imin, imax = float(in_scope[0]), float(in_scope[1])
    omin, omax, ostep = (float(v) for v in out_scope)
    n = out_size(omin, omax, ostep)
    v = (omin + ostep / 2) + torch.arange(n, dtype=torch.float64) * ostep
    g = (v - imin) / (imax - imin) * 2 - 1
    pos = ((g + 1) * size - 1) / 2
    i0 = pos.floor()
    return i0.long(), (i0 + 1) - pos, pos - i0


def _taps(in_scope, out_scope, size):
    """-> [(index clamped into the map [n], weight [n], zero where the index is outside)] for the two neighbours."""
    i0, w0, w1 = axis64(in_scope, out_scope, size)
    taps = []
    for i, w in ((i0, w0), (i0 + 1, w1)):
        inside = (i >= 0) & (i < size)
        taps.append((i.clamp(0, size - 1), torch.where(inside, w, torch.zeros_like(w))))
    return taps


def resample64(x, input_scope, output_scope, absolute=False):
    """x [B, C, h, w] -> [B, C, H, W]: sum over the four neighbours of weight_row * weight_col * value, zero outside.
    ``absolute``: sum of |weight| |value| instead -- the blend's normaliser (the weights are non-negative)."""
    x = _d(x)
    if absolute:
        x = x.abs()
    rows = _taps(input_scope[0], output_scope[0], x.shape[-2])
    cols = _taps(input_scope[1], output_scope[1], x.shape[-1])
    out = 0.0
    for ri, rw in rows:
        for ci, cw in cols:
            out = out + x[..., ri, :][..., ci] * (rw.view(-1, 1) * cw.view(1, -1))
    return out


def padded_mask(input_scope, output_scope, hw):
    """[H, W] bool: output pixels none of whose four neighbours lies inside the map (exactly zero in every implementation)."""
    live = []
    for i_s, o_s, size in zip(input_scope, output_scope, hw):
        i0, _, _ = axis64(i_s, o_s, size)
        live.append(((i0 >= 0) & (i0 < size)) | ((i0 + 1 >= 0) & (i0 + 1 < size)))
    return ~(live[0].view(-1, 1) & live[1].view(1, -1))


def features64(x, sd, input_scope, output_scope, prefix=""):
    """The head up to the last layer's input: transform, then classifier.{0,1,2} and .{3,4,5}.  NCHW."""
    y = resample64(x, input_scope, output_scope)
    for conv, bn in (("classifier.0.", "classifier.1."), ("classifier.3.", "classifier.4.")):
        y = F.relu(bn64(F.conv2d(y, _d(sd[prefix + conv + "weight"]), padding=1), sd, prefix + bn))
    return y


def logits64(feat, weight, bias, absolute=False):
    """classifier.6: feat [B, C, H, W], weight [K, C(, 1, 1)], bias [K] -> [B, K, H, W]; ``absolute``: sum |w| |x| + |b|."""
    w, b, feat = _d(weight).reshape(len(bias), -1), _d(bias), _d(feat)
    if absolute:
        w, b, feat = w.abs(), b.abs(), feat.abs()
    return torch.einsum("kc,bchw->bkhw", w, feat) + b.view(1, -1, 1, 1)


def sigmoid64(z):
    return 1.0 / (1.0 + torch.exp(-_d(z)))


def entropy64(z):
    """Binary entropy of sigmoid(z) in nats, per element: -(p ln p + (1 - p) ln(1 - p)).  It is even in z; with a = |z| and
    t = exp(-a) it is log1p(t) + a t / (1 + t): no cancellation and no overflow."""
    a = _d(z).abs()
    t = torch.exp(-a)
    return torch.log1p(t) + a * t / (1.0 + t)


def head64(x, sd, input_scope, output_scope, prefix=""):
    """-> dict(logits, prob [B, K, X, Y], entropy_sum [B, K], area [B, K] int64)."""
    feat = features64(x, sd, input_scope, output_scope, prefix)
    z = logits64(feat, sd[prefix + "classifier.6.weight"], sd[prefix + "classifier.6.bias"])
    p = sigmoid64(z)
    return dict(features=feat, logits=z, prob=p, entropy_sum=entropy64(z).sum((-2, -1)), area=(p > 0.5).sum((-2, -1)))


def head_abs64(x, sd, input_scope, output_scope, prefix=""):
    """The abs chain of the head: (normaliser of the last layer's input, normaliser of the logits).  The blend's weights are
    non-negative and ReLU passes magnitudes on, so the yardstick itself on |x| with ``abs_state`` is the chain."""
    a = abs_state({k: v for k, v in sd.items() if k.startswith(prefix)})
    a[prefix + "classifier.6.bias"] = _d(sd[prefix + "classifier.6.bias"]).abs()
    feat = features64(_d(x).abs(), a, input_scope, output_scope, prefix)
    return feat, logits64(feat, a[prefix + "classifier.6.weight"], a[prefix + "classifier.6.bias"])
