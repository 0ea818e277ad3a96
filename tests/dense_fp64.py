"""Float64 references of the dense layers and of the token MLP, with the normaliser the suite's gates use
(test_dense_gpu.py::test_conv2d_f16x3_is_fp32_class): per output element the sum of |a*b| over the products -- and, with
an epilogue, |scale| times that plus |shift| (the abs chain, as tests/spconv_fp64.py builds it for the sparse layers).

Gate of a split-arithmetic kernel (f16x3, bf16x6): e = max |got - ref| / norm <= 1.5e-6, and e <= 3 e_f32 + 1e-8 with
e_f32 from the f32-input MFMA kernel on the same input."""
import torch
import torch.nn.functional as F

E_MAX = 1.5e-6


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _epilogue(y, nrm, scale, shift, relu):
    if scale is not None:
        y, nrm = y * scale.double().view(1, -1, 1, 1), nrm * scale.double().abs().view(1, -1, 1, 1)
    if shift is not None:
        y, nrm = y + shift.double().view(1, -1, 1, 1), nrm + shift.double().abs().view(1, -1, 1, 1)
    if relu:
        y = torch.where(y <= 0, torch.zeros_like(y), y)
    return nhwc(y), nhwc(nrm)


def conv_fp64(x, w, stride, pad, scale=None, shift=None, relu=False):
    """x [B,Cin,H,W], w [Cout,Cin,k,k] (CPU) -> (ref, norm) in NHWC, float64."""
    y = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    nrm = F.conv2d(x.abs().double(), w.abs().double(), stride=stride, padding=pad)
    return _epilogue(y, nrm, scale, shift, relu)


def deconv_fp64(x, w, scale=None, shift=None, relu=False):
    """The 2x2 stride-2 transposed convolution: x [B,Cin,H,W], w [Cin,Cout,2,2] -> (ref, norm) in NHWC, float64."""
    y = F.conv_transpose2d(x.double(), w.double(), stride=2)
    nrm = F.conv_transpose2d(x.abs().double(), w.abs().double(), stride=2)
    return _epilogue(y, nrm, scale, shift, relu)


def err(got, ref, norm):
    return float(((got.detach().cpu().double() - ref).abs() / norm).max())


def check_split_gate(e, e32, what=""):
    assert e32 < E_MAX and e < E_MAX and e < 3.0 * e32 + 1e-8, f"{what}: e = {e:.3e}, e_f32 = {e32:.3e}"


def mlp_fp64(x, ln_w, ln_b, w1, b1, w2, b2, eps=1e-5):
    """x + fc2(GELU(fc1(LN(x)))) in float64 (exact GELU), x [T, C]."""
    xd = x.double()
    xn = F.layer_norm(xd, (x.shape[1],), ln_w.double(), ln_b.double(), eps)
    return xd + F.gelu(xn @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()
