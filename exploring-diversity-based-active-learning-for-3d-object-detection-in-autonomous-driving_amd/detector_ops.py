"""Device-side detector primitives (torch tensors in, HIP kernels underneath).

Activations are NHWC float32.  Weight packing helpers turn reference-layout
parameters (``Conv2d.weight [Cout,Cin,k,k]``, ``ConvTranspose2d.weight [Cin,Cout,2,2]``,
eval ``BatchNorm2d``) into the kernel layouts once, outside the hot loop.
"""
import ctypes
from typing import NamedTuple

import torch

from . import lib
from .selector_ops import _dev, _ptr, _stream


# ------------------------------------------------------------------ packing (one-off)
def pack_conv_weight(w):
    """[Cout,Cin,k,k] -> [Cout,k*k,Cin] contiguous."""
    co, ci, kh, kw = w.shape
    return w.detach().permute(0, 2, 3, 1).reshape(co, kh * kw, ci).contiguous().float()


def pack_deconv_weight(w):
    """ConvTranspose2d [Cin,Cout,2,2] -> [Cout,4,Cin] with tap = dy*2+dx."""
    ci, co, kh, kw = w.shape
    assert kh == 2 and kw == 2
    return w.detach().permute(1, 2, 3, 0).reshape(co, 4, ci).contiguous().float()


def fold_bn(bn, bias=None):
    """eval BatchNorm -> (scale, shift): y = x*scale + shift.  ``bias``: the bias of the layer in front of it, folded in as
    (x + b) * s + t in float32 on the rounded scale and shift."""
    inv = torch.rsqrt(bn.running_var.detach().double() + bn.eps)
    g = bn.weight.detach().double() if bn.weight is not None else torch.ones_like(inv)
    b = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(inv)
    scale = g * inv
    shift = b - bn.running_mean.detach().double() * scale
    scale, shift = scale.float().contiguous(), shift.float().contiguous()
    if bias is not None:
        shift = shift + bias.detach().float().to(scale.device) * scale
    return scale, shift


def fold_conv_bn(pairs, swap_hw=False, first=0, pad_cin=False, deconv=False):
    """[(conv, eval BatchNorm2d or None)] reading ONE input -> (w [Cout_total, taps, Cin] f32, scale, shift) of the single
    launch with their output channels side by side: y = conv(x, w) * scale + shift (no BatchNorm: scale 1, shift 0; a
    conv bias is folded as ``fold_bn`` does).  ``swap_hw``: the kernels' two spatial axes swapped (the map is [y, x], the
    weights [x, y]); ``first``: the map holds the input channels rotated, [channels first: | channels :first];
    ``pad_cin``: Cin zero-padded to a multiple of 16 (the matrix-core kernels' step; the caller pads the map);
    ``deconv``: ConvTranspose2d 2x2 weights (``pack_deconv_weight``).  Pure torch, on the parameters' device."""
    ws, scales, shifts = [], [], []
    for conv, bn in pairs:
        w = conv.weight.detach().float()
        if bn is not None:
            scale, shift = fold_bn(bn, conv.bias)
        else:
            scale = torch.ones(conv.out_channels, device=w.device)
            shift = torch.zeros(conv.out_channels, device=w.device)
            if conv.bias is not None:
                shift = shift + conv.bias.detach().float() * scale
        if swap_hw:
            w = w.transpose(2, 3)
        if first:
            w = torch.cat([w[:, first:], w[:, :first]], dim=1)
        ws.append(pack_deconv_weight(w) if deconv else pack_conv_weight(w))
        scales.append(scale)
        shifts.append(shift)
    w = torch.cat(ws)
    if pad_cin and w.shape[2] % 16:
        w = torch.nn.functional.pad(w, (0, 16 - w.shape[2] % 16))
    return w, torch.cat(scales), torch.cat(shifts)


def split_bf16x3(w_packed):
    """f32 packed weights (device) -> bf16 [3, *shape] exact three-way split (hi, mid, lo)."""
    w = _dev(w_packed, torch.float32, "w")
    out = torch.empty((3,) + tuple(w.shape), dtype=torch.bfloat16, device=w.device)
    lib.call("al3d_split_bf16x3", _ptr(w), w.numel(), _ptr(out), _stream())
    return out


def split_f16x3(w_packed, scale=None):
    """f32 packed weights (device) -> (f16 [2, *shape] planes (wh, wl), scale * 2^-s).

    ``s`` is the power of two that brings max|w| just under 2^14 (f16's exponent range is spent
    on the weights once, here, so the kernel never depends on it); it is folded back into the
    per-channel scale the kernel multiplies its accumulator with -- exact."""
    import math
    w = _dev(w_packed, torch.float32, "w")
    amax = float(w.abs().max()) if w.numel() else 0.0
    if not math.isfinite(amax):
        raise lib.Al3dError("split_f16x3: non-finite weight")
    s = 14 - math.frexp(amax)[1] if amax > 0.0 else 0          # amax <= 2^e  ->  amax * 2^s <= 2^14
    s = max(-100, min(100, s))
    out = torch.empty((2,) + tuple(w.shape), dtype=torch.float16, device=w.device)
    lib.call("al3d_split_f16x3", _ptr(w), w.numel(), s, _ptr(out), _stream())
    cout = w.shape[0]
    base = torch.ones(cout, dtype=torch.float32, device=w.device) if scale is None else \
        _dev(scale, torch.float32, "scale")
    return out, (base.double() * 2.0 ** (-s)).float().contiguous()


# Arithmetic of the MFMA conv kernels (AL3D_MATH):
#   "f16x3"  (default) three f16 products per MAC (fp32-class, activations < 65504) in the dense
#            neck + head and in the sparse encoder
#   "bf16x6" fp32-faithful six-product split on the bf16 matrix cores everywhere (full fp32 range)
#   "f32"    fp32-input MFMA (bitwise an fp32 FMA chain)
#   "auto"   f16x3, and the sweep re-runs under bf16x6 each batch whose embeddings left the f16x3 range
#            (MATH reads "f16x3", MATH_AUTO is set: sweep.sweep_embeddings(recover_range=None))
import os as _os
MATH = _os.environ.get("AL3D_MATH", "f16x3")
MATH_AUTO = MATH == "auto"
if MATH_AUTO:
    MATH = "f16x3"
if MATH not in ("f16x3", "bf16x6", "f32"):
    raise lib.Al3dError(f"AL3D_MATH={MATH!r}: expected f16x3, bf16x6, f32 or auto")



# structure of the f16x3 dense kernels: "auto" = 3x3/s1 layers on the fragment-streamed halo kernel, every other
# geometry (stride-2 entry, 1x1 / deconv deblocks, fused head) on the LDS-DMA kernel; "stream" = round 1's policy
# (generic launches with >= 24 steps stream their weights in fragment order, the others stage both tiles through
# LDS), "bstream" = streamed weights everywhere, "frag" = only the 3x3 layers, "lds" = the LDS-staged kernels
# everywhere.  The same bits in all of them; kept for A/B
DENSE = _os.environ.get("AL3D_DENSE", "auto")


class F16x3Packed:
    """f16x3 weights in MFMA fragment order for the kernels that stream them from L2.
    kind "frag3x3": [2,Cout/32,Cin/16,9,64,8] (3x3/s1/p1); kind "bstream": [2,ceil(Cout/128)*4,taps,
    Cin/16,64,8] (any other geometry, zero rows beyond Cout)."""
    dtype = torch.float16

    def __init__(self, kind, data, cout, taps, cin):
        self.kind, self.data, self.cout, self.taps, self.cin = kind, data, cout, taps, cin


def pack_frag_f16x3(planes):
    """f16 planes [2,Cout,9,Cin] -> fragment order for the 3x3/s1/p1 kernel (every wave streams its B
    operands from L2, no LDS staging of weights)."""
    planes = _dev(planes, torch.float16, "planes")
    _, cout, taps, cin = planes.shape
    assert taps == 9
    out = torch.empty((2, cout // 32, cin // 16, 9, 64, 8), dtype=torch.float16, device=planes.device)
    lib.call("al3d_pack_f16x3_frag", _ptr(planes), cout, cin, _ptr(out), _stream())
    return F16x3Packed("frag3x3", out, cout, 9, cin)


def pack_frag16_f16x3(planes):
    """f16 planes [2,Cout,9,Cin] -> 16x16x32 fragment order for the 3x3/s1/p1 kernel on the narrow MFMA shape."""
    planes = _dev(planes, torch.float16, "planes")
    _, cout, taps, cin = planes.shape
    assert taps == 9
    out = torch.empty((2, cout // 16, cin // 32, 9, 64, 8), dtype=torch.float16, device=planes.device)
    lib.call("al3d_pack_f16x3_frag16", _ptr(planes), cout, cin, _ptr(out), _stream())
    return F16x3Packed("frag16", out, cout, 9, cin)


def pack_bstream_f16x3(planes):
    """f16 planes [2,Cout,taps,Cin] -> fragment order for the streamed-weight kernel of the other geometries."""
    planes = _dev(planes, torch.float16, "planes")
    _, cout, taps, cin = planes.shape
    n = lib.load().al3d_pack_f16x3_bstream_elems(cout, taps, cin)
    if n <= 0:
        raise lib.Al3dError(f"pack_bstream_f16x3: unsupported shape Cout={cout} taps={taps} Cin={cin}")
    out = torch.empty((2, (cout + 127) // 128 * 4, taps, cin // 16, 64, 8), dtype=torch.float16,
                      device=planes.device)
    assert out.numel() == n
    lib.call("al3d_pack_f16x3_bstream", _ptr(planes), cout, taps, cin, _ptr(out), _stream())
    return F16x3Packed("bstream", out, cout, taps, cin)


def pack_dma_f16x3(planes):
    """f16 planes [2,Cout,taps,Cin] -> per-step LDS images for the LDS-DMA kernel of the generic geometries."""
    planes = _dev(planes, torch.float16, "planes")
    _, cout, taps, cin = planes.shape
    n = lib.load().al3d_pack_f16x3_bstream_elems(cout, taps, cin)
    if n <= 0:
        raise lib.Al3dError(f"pack_dma_f16x3: unsupported shape Cout={cout} taps={taps} Cin={cin}")
    out = torch.empty(((cout + 127) // 128, taps, cin // 16, 2, 128, 16), dtype=torch.float16, device=planes.device)
    assert out.numel() == n
    lib.call("al3d_pack_f16x3_dma", _ptr(planes), cout, taps, cin, _ptr(out), _stream())
    return F16x3Packed("dma", out, cout, taps, cin)


def pack_wino_f16x3(w_packed, scale=None):
    """f32 packed 3x3 weights [Cout, 9, Cin] -> Winograd F(2x2, 3x3) weights U = G g G^T (float64 on the host side of the
    split, then the usual f16x3 planes) in fragment order for ``al3d_conv3x3_nhwc_f16x3_wino``, + the scale to hand it."""
    w = _dev(w_packed, torch.float32, "w")
    cout, taps, cin = w.shape
    assert taps == 9
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=w.device)
    U = torch.einsum("ak,okqc,bq->oabc", G, w.double().view(cout, 3, 3, cin), G).reshape(cout, 16, cin).float().contiguous()
    planes, scale = split_f16x3(U, scale)
    out = torch.empty((2, cout // 32, cin // 16, 16, 64, 8), dtype=torch.float16, device=w.device)
    lib.call("al3d_pack_f16x3_wino", _ptr(planes), cout, cin, _ptr(out), _stream())
    return F16x3Packed("wino", out, cout, 9, cin), scale


def wino_ok(cout, cin, ksize, stride, pad):
    return (ksize, stride, pad) == (3, 1, 1) and cout % 64 == 0 and cin % 16 == 0


def pack_glds_f16x3(planes):
    """f16 planes [2,Cout,K,Cin] (split_f16x3 of the [Cout,K,Cin] weights) -> the LDS image order of the DMA-gather
    kernels (al3d_sp_pack_glds_f16x3: [K][Cin/16][2][ceil32(Cout)][16] f16, halves swizzled)."""
    planes = _dev(planes, torch.float16, "planes")
    _, cout, K, cin = planes.shape
    n = lib.load().al3d_sp_pack_glds_f16x3_elems(cout, K, cin)
    if n <= 0:
        raise lib.Al3dError(f"pack_glds_f16x3: unsupported shape Cout={cout} K={K} Cin={cin}")
    out = torch.empty((n,), dtype=torch.float16, device=planes.device)
    lib.call("al3d_sp_pack_glds_f16x3", _ptr(planes), cout, K, cin, _ptr(out), _stream())
    return out


def frag_ok(cout, cin, ksize, stride, pad):
    return ksize == 3 and stride == 1 and pad == 1 and cout % 128 == 0 and cin % 32 == 0


# sparse-conv structure.  f16x3: "auto" = per channel pair whichever kernel measured fastest on the real rulebooks
# (RNG_PAIRS: range-gather LDS-DMA kernel for the 27-tap submanifold layers; GLDS_PAIRS: per-tap LDS-DMA gather; else
# the register-gather wave kernel), "glds" / "wave2" = one of those everywhere, "rng" = range gather wherever built
# (same bits in all of them for Cin <= 32; see al3d_sp_conv_rng_f16x3 for Cin = 64).  bf16x6: "auto" = the software-pipelined wave kernel; "wave" (unpipelined
# wave kernel) and "tile" (LDS-staged 128-row tile) give the same bits, for A/B
SPCONV = _os.environ.get("AL3D_SPCONV", "auto")
GLDS_PAIRS = {(32, 32), (64, 64)}
if _os.environ.get("AL3D_GLDS_PAIRS"):           # dev override, e.g. "32x32,64x64,128x128"
    GLDS_PAIRS = {tuple(int(v) for v in t.split("x")) for t in _os.environ["AL3D_GLDS_PAIRS"].split(",")}


# row format of the f16x3 sparse encoder's activations between layers (csrc/sp_rows.h): "pair" = the two f16 planes
# of the arithmetic, split once in the producer's epilogue; "f32" = plain rows, split per gathered (row, tap)
SPROWS = _os.environ.get("AL3D_SPROWS", "pair")
# the same format for the dense neck's maps where the consumer is the LDS-DMA kernel (block outputs -> stride-2 conv /
# deblocks, concat map -> fused head): "pair" | "f32"
DPIX = _os.environ.get("AL3D_DPIX", "pair")
IO_IN_PAIR, IO_OUT_PAIR, IO_RES_PAIR = 1, 2, 4
# what the sparse encoder hands the dense neck: "rows" = its last level's rows + a BEV row index (BevRows; the neck's
# first 3x3 reads them in place and skips its empty halo rows), where neck_rows_ok allows it; "dense" = always the
# zero-filled [B,H,W,C*D] map.  The same bits
NECK_IN = _os.environ.get("AL3D_NECK_IN", "rows")
if NECK_IN not in ("rows", "dense"):
    raise lib.Al3dError(f"AL3D_NECK_IN={NECK_IN!r}: expected rows or dense")


def neck_rows_ok(kind, depth=2, channels=8):
    """May the neck's first conv (dense structure ``kind``) read the encoder's last level (``depth`` z levels of
    ``channels``-wide rows) as BevRows?  Only the streamed 3x3 f16x3 kernel has the rows input, for two z levels."""
    return NECK_IN == "rows" and MATH == "f16x3" and kind == "frag3x3" and depth == 2 and channels % 8 == 0


class BevRows:
    """The sparse encoder's last level in place of its dense BEV map: ``rows`` [n, C] f32, ``coords`` [n, 4] i32
    (b, z, y, x), ``index`` [B, H, W, D] i32 (row of (pixel, z), -1 = none; ``bev_index``).  ``shape`` is the map's,
    (B, H, W, C*D) with channel = c*D + z; ``dense()`` materialises it.  ``conv2d_nhwc`` takes it where
    ``neck_rows_ok`` holds."""

    def __init__(self, rows, coords, index):
        self.rows, self.coords, self.index = rows, coords, index
        B, H, W, Dz = index.shape
        self.shape = (B, H, W, rows.shape[1] * Dz)
        self.device = rows.device

    def dense(self):
        B, H, W, Dz = self.index.shape
        out = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        lib.call("al3d_sp_to_dense_nhwc", _ptr(self.rows), _ptr(self.coords), self.rows.shape[0], self.rows.shape[1],
                 B, Dz, H, W, _ptr(out), _stream())
        return out


def bev_index(coords, n, batch_size, shape):
    """[B, H, W, D] i32 row index of a level's n rows (coords [n, 4] i32; shape = (D, H, W), D = 2)."""
    Dz, H, W = (int(s) for s in shape)
    idx = torch.empty((batch_size, H, W, Dz), dtype=torch.int32, device=coords.device)
    lib.call("al3d_sp_fill_i32", _ptr(idx), idx.numel(), -1, _stream())
    lib.call("al3d_sp_bev_index", _ptr(coords), n, batch_size, Dz, H, W, _ptr(idx), _stream())
    return idx


def rows_convert(x, to_pair):
    """[n, C] f32 rows <-> pair rows (same shape and dtype; C % 8 == 0)."""
    x = _dev(x, torch.float32, "x")
    out = torch.empty_like(x)
    lib.call("al3d_sp_rows_convert_f16x3", _ptr(x), x.shape[0], x.shape[1], 1 if to_pair else 0, _ptr(out), _stream())
    return out


# the range-gather form of the LDS-DMA kernel (27-tap submanifold layers of these channel pairs; "rng" = wherever it
# is built, "auto" = RNG_PAIRS, measured)
RNG_BUILT = {(32, 32), (64, 64)}
RNG_PAIRS = {(32, 32)}        # measured: ahead of the per-tap kernel at 32 channels, behind at 64
if _os.environ.get("AL3D_RNG_PAIRS") is not None:   # dev override, e.g. "32x32,64x64" or "" for none
    RNG_PAIRS = {tuple(int(v) for v in t.split("x")) for t in _os.environ["AL3D_RNG_PAIRS"].split(",") if t}


# Block-staged kernel (csrc/spconv_blk.hip): 27-tap submanifold layers of these channel pairs stage the union of a
# 128-row chunk's neighbourhoods once; the encoder then numbers the level's rows column by column
# (al3d_sp_down_sites_blocked).  Built, bit-identical, and MEASURED SLOWER than the range / per-tap kernels on lidar
# data (round 5, DESIGN 5.3: fragment reads through arbitrary local indices are LDS-bank-conflict bound, and column order
# makes 91 % instead of 72 % of the (tile, tap) pairs live), so no pair takes it by default.
# AL3D_BLK_PAIRS: opt-in, e.g. "32x32,64x64,128x128"
BLK_BUILT = {(32, 32), (64, 64), (128, 128)}
BLK_PAIRS = set()
if _os.environ.get("AL3D_BLK_PAIRS") is not None:
    BLK_PAIRS = {tuple(int(v) for v in t.split("x")) for t in _os.environ["AL3D_BLK_PAIRS"].split(",") if t}


# Tap-mask row order (al3d_sp_mask_window_sort): levels whose 27-tap submanifold layers have these output widths get their rows
# re-numbered by neighbour mask inside windows of MASK_SORT_WINDOW raster rows, so that the rows of a 32-row tile lack the same
# taps (the per-tap gather kernels of the 64- and 128-channel levels execute 10-15 % fewer (tile, tap) pairs: 64 -> 64 layers
# -11 %, 128 -> 128 -10 %, bench +2.3 % at windows of 16384; level 1's range-gather kernel needs raster order: +9 % slower
# there).  AL3D_MASK_SORT: e.g. "64,128" / "" for none; AL3D_MASK_SORT_WINDOW: 1024 | 4096 | 8192 | 16384
MASK_SORT = {64, 128}
if _os.environ.get("AL3D_MASK_SORT") is not None:
    MASK_SORT = {int(v) for v in _os.environ["AL3D_MASK_SORT"].split(",") if v}
MASK_SORT_WINDOW = int(_os.environ.get("AL3D_MASK_SORT_WINDOW", "16384"))
MASK_SORT_WINDOWS = {}         # per width, e.g. AL3D_MASK_SORT_WINDOWS="64:4096,128:16384" (else MASK_SORT_WINDOW for all)
if _os.environ.get("AL3D_MASK_SORT_WINDOWS"):
    MASK_SORT_WINDOWS = {int(a): int(b) for a, b in (t.split(":") for t in _os.environ["AL3D_MASK_SORT_WINDOWS"].split(",") if t)}


BLK_ORDER_ONLY = _os.environ.get("AL3D_BLK_ORDER_ONLY", "0") == "1"   # dev: column order for these pairs' levels, old kernels


class BlkPlan:
    """Per-level plan of the block-staged kernel (al3d_sp_block_plan): chunk headers, staged row lists, local indices."""

    def __init__(self, hdr, rows, loc, R, cap):
        self.hdr, self.rows, self.loc, self.R, self.cap = hdr, rows, loc, R, cap


def block_shape(cin, cout):
    import ctypes
    R, cap = ctypes.c_int(0), ctypes.c_int(0)
    lib.call("al3d_sp_block_shape", cin, cout, ctypes.byref(R), ctypes.byref(cap))
    return R.value, cap.value


def block_plan(nbr, n_out, cin, cout):
    """Plan of a tiled 27-tap table for the block-staged kernel of cin -> cout."""
    dev = nbr.device
    R, cap = block_shape(cin, cout)
    chunks = (max(n_out, 1) + R - 1) // R
    hdr = torch.empty((chunks, 2), dtype=torch.int32, device=dev)
    rows = torch.empty((chunks, cap), dtype=torch.int32, device=dev)
    loc = torch.empty((chunks, 27, R), dtype=torch.int16, device=dev)
    lib.call("al3d_sp_block_plan", _ptr(nbr), nbr.shape[1], 27, n_out, R, cap, _ptr(hdr), _ptr(rows), _ptr(loc), _stream())
    return BlkPlan(hdr, rows, loc, R, cap)


# Level-0 layers (16 input channels, 27 taps) on raster-ordered rows (csrc/spconv_l0.hip): AL3D_L0 = "raster"
# (default: the encoder renumbers the voxelizer's rows in raster order and runs these layers as item streams with
# LDS-resident weights) | "off" (first-appearance order, register-gather kernel: round 3's path).  R16_COUTS: the output
# widths that take the item-stream kernel (16: the five submanifold layers; 32: the strided 16 -> 32 layer)
L0 = _os.environ.get("AL3D_L0", "raster")
if L0 not in ("raster", "off"):
    raise lib.Al3dError(f"AL3D_L0={L0!r}: expected raster or off")
R16_COUTS = {16}
if _os.environ.get("AL3D_R16_COUTS") is not None:    # dev override, e.g. "16,32" or "" for none
    R16_COUTS = {int(v) for v in _os.environ["AL3D_R16_COUTS"].split(",") if v}
R16_TPW = int(_os.environ.get("AL3D_R16_TPW", "0"))   # tiles per wave (0: the library's default)
# row format between two item-stream layers of level 0: "f32" (default: the encoder's output keeps the bits of every other
# kernel structure and of round 3) | "pair" (the split runs once, in the producer: -9 % per layer at 32 frames per launch,
# nothing measurable end to end, and the stored activations lose 1-2 bits: embedding moves by <= 9.5e-7 of its scale)
L0_ROWS = _os.environ.get("AL3D_L0_ROWS", "f32")


def sparse_raster():
    """True when the encoder renumbers its level-0 rows in raster order."""
    return MATH == "f16x3" and SPCONV == "auto" and L0 == "raster"


def pack_r16_f16x3(planes):
    """f16 planes [2,Cout,27,16] (split_f16x3 of the [Cout,27,16] weights) -> the item-stream kernel's LDS image
    (al3d_sp_pack_r16_f16x3: [27][2 planes][2 k-halves][Cout][8] f16)."""
    planes = _dev(planes, torch.float16, "planes")
    _, cout, K, cin = planes.shape
    n = lib.load().al3d_sp_pack_r16_f16x3_elems(cout)
    if n <= 0 or K != 27 or cin != 16:
        raise lib.Al3dError(f"pack_r16_f16x3: unsupported shape Cout={cout} K={K} Cin={cin}")
    out = torch.empty((n,), dtype=torch.float16, device=planes.device)
    lib.call("al3d_sp_pack_r16_f16x3", _ptr(planes), cout, _ptr(out), _stream())
    return out


def raster_perm(coords, batch, shape, frame_rows_max=0):
    """coords [n,4] i32 (b,z,y,x) -> (perm [n] i32: raster position -> row, coords in raster order).
    frame_rows_max > 0: the rows are frame-sorted with at most that many rows per frame (the voxelizer's output and its
    voxel cap): the sort then runs in LDS, one workgroup per frame."""
    coords = _dev(coords, torch.int32, "coords")
    n = coords.shape[0]
    D_, H_, W_ = [int(v) for v in shape]
    perm = torch.empty((n,), dtype=torch.int32, device=coords.device)
    out = torch.empty_like(coords)
    ws = torch.empty(max(int(lib.load().al3d_sp_raster_perm_workspace_bytes(n, batch, D_, H_)), 1), dtype=torch.uint8,
                     device=coords.device)
    lib.call("al3d_sp_raster_perm", _ptr(coords), n, batch, D_, H_, W_, int(frame_rows_max), _ptr(ws), _ptr(perm), _ptr(out),
             _stream())
    raster_perm.last_status = ws[:4].view(torch.int32)       # device status word: see check_raster_status
    return perm, out


def check_raster_status(status):
    """Raise when al3d_sp_raster_perm found its frame_rows_max promise broken (one small D2H: call it where the
    stream is synchronised anyway)."""
    v = int(status.item()) if status is not None else 0
    if v:
        raise lib.Al3dError("sparse encoder: frame_rows_max was promised (example['voxel_cap']) but "
                            + ("the voxel rows are not frame-sorted" if v & 1 else "a frame holds more than 65,535 voxels")
                            + "; pass frame_rows_max=0 for rows in any order")


def rows_gather_pad(rows, perm, channels_out, to_pair=False):
    """out[r] = rows[perm[r]] zero-padded to channels_out channels (f32 rows or pair rows)."""
    rows = _dev(rows, torch.float32, "rows")
    n, F = rows.shape
    out = torch.empty((n, channels_out), dtype=torch.float32, device=rows.device)
    lib.call("al3d_sp_rows_gather_pad_f32", _ptr(rows), _ptr(perm), n, F, channels_out, 1 if to_pair else 0, _ptr(out), _stream())
    return out


def tile_items(nbr, n_out, tmask):
    """Item list of a tiled 27-tap table: (first [ntiles+1] i32, items [9*ntiles+1, 4] i32)."""
    dev = nbr.device
    ntiles = (max(n_out, 1) + 31) // 32
    first = torch.empty((ntiles + 1,), dtype=torch.int32, device=dev)
    items = torch.empty((9 * ntiles + 1, 4), dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.load().al3d_sp_tile_items_workspace_bytes(n_out)), dtype=torch.uint8, device=dev)
    lib.call("al3d_sp_tile_items", _ptr(nbr), nbr.shape[1], 27, n_out, _ptr(tmask), _ptr(ws), _ptr(first), _ptr(items), _stream())
    return first, items


# ------------------------------------------------------------------ sparse-conv dispatch (the encoder and sparse_conv_layer)
# The 3-D layers the matrix-core kernels are built for (others, e.g. 5 -> 16 in f32, run on the VALU kernel)
MFMA_PAIRS = {(16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128)}

# structure -> (al3d_sp_conv_* entry point, weight format, tiled table, side data).  Weight formats (sparse_pack): "kic" f32
# [K,Cin,Cout], "oki" f32 [Cout,K,Cin], "bf16x6" planes (split_bf16x3), "f16x3" planes (split_f16x3), "glds"
# (pack_glds_f16x3), "r16" (pack_r16_f16x3).  Tiled tables (pitched, + per-tile tap masks) are read by the f16x3 kernels
# with an io argument, and only those read and write pair rows.  Side data, built once per table (sparse_side): "trng"
# (al3d_sp_tile_ranges), "plan" (block_plan), "items" (tile_items).
SPARSE = {
    False: ("al3d_sp_conv_f32", "kic", False, None),
    True: ("al3d_sp_conv_mfma_f32", "oki", False, None),
    "bf16x6": ("al3d_sp_conv_bf16x6", "bf16x6", False, None),
    "wave": ("al3d_sp_conv_wave_bf16x6", "bf16x6", False, None),
    "wave2": ("al3d_sp_conv_wave2_bf16x6", "bf16x6", False, None),
    "wave2_f16x3": ("al3d_sp_conv_wave2_f16x3", "f16x3", False, None),
    "wave2_f16x3_tiles": ("al3d_sp_conv_wave2_f16x3_tiles_io", "f16x3", True, None),
    "glds_f16x3": ("al3d_sp_conv_glds_f16x3_io", "glds", True, None),
    "rng_f16x3": ("al3d_sp_conv_rng_f16x3", "glds", True, "trng"),
    "blk_f16x3": ("al3d_sp_conv_blk_f16x3", "glds", True, "plan"),
    "r16_f16x3": ("al3d_sp_conv_r16_f16x3", "r16", True, "items"),
}
# the table arguments of a tiled kernel between the pitch and K
_SIDE_ARGS = {None: lambda t: (t["tmask"],), "trng": lambda t: (t["tmask"], t["trng"]),
              "plan": lambda t: (t["tmask"], t["plan"].hdr, t["plan"].rows, t["plan"].loc),
              "items": lambda t: (t["items"][1], t["items"][0])}


def sparse_structure(cin, cout, K, subm, raster_ok):
    """(structure, input width, column order) of the sparse layer cin -> cout with K taps under the current settings.
    A narrow first layer (5 -> 16) runs zero-padded to 16 input channels on the matrix cores (not in f32).  raster_ok: the
    layer may read raster-ordered rows (the encoder's renumbered level 0: the item-stream kernel).  Column order: the
    level this submanifold layer reads is numbered column by column (the block-staged kernel, or AL3D_BLK_ORDER_ONLY)."""
    if MATH != "f32" and cin < 16 and (16, cout) in MFMA_PAIRS:
        cin = 16
    pair = (cin, cout)
    if pair not in MFMA_PAIRS:
        return False, cin, False
    if MATH == "f32":
        return True, cin, False
    if MATH == "bf16x6":
        # measured per channel pair on the real rulebooks (tools/bench_splayers.py): the software-pipelined wave kernel
        # wins everywhere; "wave" / "tile" select the older structures (same bits)
        return {"wave": "wave", "tile": "bf16x6"}.get(SPCONV, "wave2"), cin, False
    auto = SPCONV == "auto"
    cols = auto and subm and K == 27 and pair in BLK_PAIRS & BLK_BUILT
    rng = SPCONV in ("auto", "rng") and pair in (RNG_BUILT if SPCONV == "rng" else RNG_PAIRS & RNG_BUILT)
    if raster_ok and sparse_raster() and cin == 16 and K == 27 and cout in R16_COUTS:
        name = "r16_f16x3"
    elif cols and not BLK_ORDER_ONLY:
        name = "blk_f16x3"
    elif rng and subm and K == 27:
        name = "rng_f16x3"
    elif SPCONV == "glds" or rng or (auto and pair in GLDS_PAIRS):
        name = "glds_f16x3"
    else:
        name = "wave2_f16x3_tiles"
    return name, cin, cols


def sparse_pack(name, w, scale=None, cin=None):
    """Weights [K,Cin,Cout] f32 (device) -> (weights in structure `name`'s format, the scale to hand it: the f16x3 split
    folds its weight exponent into it).  cin > Cin: zero-padded input channels (sparse_structure's narrow first layer)."""
    if cin is not None and cin != w.shape[1]:
        w = torch.nn.functional.pad(w, (0, 0, 0, cin - w.shape[1]))
    fmt = SPARSE[name][1]
    if fmt == "kic":
        return w.contiguous(), scale
    w = w.permute(2, 0, 1).contiguous()
    if fmt == "oki":
        return w, scale
    if fmt == "bf16x6":
        return split_bf16x3(w), scale
    planes, scale = split_f16x3(w, scale)
    return {"glds": pack_glds_f16x3, "r16": pack_r16_f16x3}.get(fmt, lambda p: p)(planes), scale


def _i3(v):
    import ctypes
    return (ctypes.c_int * 3)(*[int(x) for x in v])


def sparse_table(tiled, coords, n, batch, dims, grid, k, stride=None, pad=None):
    """Tap-major table of the n output sites `coords` of a layer with kernel k: submanifold (stride None: the sites are the
    input level's) or strided (stride, pad); dims and grid [batch, *dims] are the input level's.  tiled: pitched, with
    per-tile tap masks.  -> dict(nbr [K, pitch | max(n, 1)] i32, n, K, tmask | None): a rulebook entry, side data goes in too."""
    K = int(k[0]) * int(k[1]) * int(k[2])
    dev = coords.device
    if tiled:
        pitch = lib.load().al3d_sp_table_pitch(n)
        nbr = torch.empty((K, pitch), dtype=torch.int32, device=dev)
        tmask = torch.empty((pitch // 32,), dtype=torch.int32, device=dev)
        out = (_ptr(nbr), pitch, _ptr(tmask))
    else:
        nbr, tmask = torch.empty((K, max(n, 1)), dtype=torch.int32, device=dev), None
        out = (_ptr(nbr),)
    if stride is None:
        fn, geom = "al3d_sp_subm_table", (batch, *dims, _ptr(grid), *k)
    else:
        fn, geom = "al3d_sp_down_table", (_i3(k), _i3(stride), _i3(pad), batch, *dims, _ptr(grid))
    lib.call(fn + ("_tiles" if tiled else ""), _ptr(coords), n, *geom, *out, _stream())
    return dict(nbr=nbr, n=n, K=K, tmask=tmask)


def sparse_side(name, tab, cin, cout):
    """Adds to table `tab` (sparse_table's) the side data structure `name` reads, unless it holds it already: one build
    per table, shared by the layers of a level."""
    side = SPARSE[name][3]
    if side is None or side in tab:
        return
    nbr, n = tab["nbr"], tab["n"]
    if side == "trng":          # (lo, len) of every (tile, kz, ky) group
        tab["trng"] = torch.empty((max(nbr.shape[1] // 32, 1), 9, 2), dtype=torch.int32, device=nbr.device)
        lib.call("al3d_sp_tile_ranges", _ptr(nbr), nbr.shape[1], tab["K"], n, _ptr(tab["trng"]), _stream())
    elif side == "plan":
        tab["plan"] = block_plan(nbr, n, cin, cout)
    else:
        tab["items"] = tile_items(nbr, n, tab["tmask"])


def sparse_down_sites(coords, n, k, stride, pad, batch, odims, grid_out, cols=False):
    """Output sites of a strided conv over the n input sites `coords`, numbered in raster (b, z, y, x) order, or column by
    column (al3d_sp_down_sites_blocked); grid_out [batch, *odims] (all -1) gets their rows.  One small D2H.
    -> coords_out [n_out, 4] i32"""
    dev = coords.device
    cap = min(n * int(k[0]) * int(k[1]) * int(k[2]), batch * int(odims[0]) * int(odims[1]) * int(odims[2]))
    out = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    fn = "al3d_sp_down_sites_blocked" if cols else "al3d_sp_down_sites"
    ws = torch.empty(getattr(lib.load(), fn + "_workspace_bytes")(batch, *odims), dtype=torch.uint8, device=dev)
    lib.call(fn, _ptr(coords), n, _i3(k), _i3(stride), _i3(pad), batch, *odims, _ptr(grid_out), _ptr(out), _ptr(counter),
             cap, _ptr(ws), _stream())
    return out[:int(counter.item())]


def sparse_launch(name, feats, tab, w, cin, cout, scale, shift, residual, relu, out, io=0):
    """The one launch of every structure: out [n, Cout] = conv of feats [*, cin] over table `tab` (with its side data),
    * scale + shift (+ residual) (ReLU).  w, scale: sparse_pack's.  io: IO_* flags (pair rows)."""
    fn, _, tiled, side = SPARSE[name]
    if io and not tiled:
        raise lib.Al3dError(f"sparse conv {name!r}: pair rows exist for the tiled f16x3 kernels only")
    nbr = tab["nbr"]
    lead = (nbr.shape[1], *[_ptr(t) for t in _SIDE_ARGS[side](tab)]) if tiled else ()
    tail = ((io, R16_TPW) if side == "items" else (io,)) if tiled else ()
    lib.call(fn, _ptr(feats), _ptr(nbr), *lead, tab["K"], _ptr(w), cin, cout, _ptr(scale), _ptr(shift), _ptr(residual),
             1 if relu else 0, _ptr(out), tab["n"], *tail, _stream())


# ------------------------------------------------------------------ dense-conv dispatch (neck, heads, camera-branch convs)
def _f16x3_packer(pack=None):
    """(f32 packed weights, scale) -> (the f16x3 planes, or pack(planes), the scale to hand the kernel)."""
    def packer(w_packed, scale):
        planes, scale = split_f16x3(w_packed, scale)
        return (planes if pack is None else pack(planes)), scale
    return packer


class DenseKind(NamedTuple):
    conv: str        # al3d_* entry point of the convolution
    deconv: str      # ... of the 2x2 / stride-2 transposed convolution, None: the structure has none
    generic: bool    # the launch takes (ksize, stride, pad); False: 3x3 / stride 1 / pad 1 only
    io: int          # the IO_* bits (pair pixels) the entry points accept; nonzero: they take an io argument
    gap: object      # fused GAP: None, "entry" (the entry points named ..._gap) or "arg" (a gap argument, may be null)
    pack: object     # (f32 packed weights [Cout,taps,Cin], scale) -> (weights, scale) for the entry points


# structure -> what its launch takes.  "f32" / "bf16x6" / "f16x3" weights are plain tensors (f32 [Cout,taps,Cin], bf16
# [3,...] planes, f16 [2,...] planes: the LDS-staged kernels), the others F16x3Packed of that kind
DENSE_KINDS = {
    "f32": DenseKind("al3d_conv2d_nhwc_f32", "al3d_deconv2x2_nhwc_f32", True, 0, None, lambda w, scale: (w, scale)),
    "bf16x6": DenseKind("al3d_conv2d_nhwc_bf16x6", "al3d_deconv2x2_nhwc_bf16x6", True, 0, None,
                        lambda w, scale: (split_bf16x3(w), scale)),
    "f16x3": DenseKind("al3d_conv2d_nhwc_f16x3", "al3d_deconv2x2_nhwc_f16x3", True, 0, "entry", _f16x3_packer()),
    "frag3x3": DenseKind("al3d_conv3x3_nhwc_f16x3_frag_io", None, False, IO_OUT_PAIR, None, _f16x3_packer(pack_frag_f16x3)),
    "frag16": DenseKind("al3d_conv3x3_nhwc_f16x3_frag16", None, False, 0, None, _f16x3_packer(pack_frag16_f16x3)),
    "wino": DenseKind("al3d_conv3x3_nhwc_f16x3_wino", None, False, IO_OUT_PAIR, None, pack_wino_f16x3),
    "bstream": DenseKind("al3d_conv2d_nhwc_f16x3_bstream", "al3d_deconv2x2_nhwc_f16x3_bstream", True, 0, None,
                         _f16x3_packer(pack_bstream_f16x3)),
    "dma": DenseKind("al3d_conv2d_nhwc_f16x3_dma", "al3d_deconv2x2_nhwc_f16x3_dma", True, IO_IN_PAIR | IO_OUT_PAIR, "arg",
                     _f16x3_packer(pack_dma_f16x3)),
}


def dense_structure(cout, cin, ksize=None, stride=None, pad=None):
    """Kind (DENSE_KINDS) of the dense layer cin -> cout under MATH / DENSE.  ksize="deconv": the 2x2 transposed conv;
    ksize=None (no geometry given): the plain weight format of MATH."""
    if MATH != "f16x3":
        return MATH
    if ksize is None or DENSE == "lds":
        return "f16x3"
    conv = ksize != "deconv"
    if DENSE == "wino" and conv and wino_ok(cout, cin, ksize, stride, pad):
        return "wino"
    if conv and frag_ok(cout, cin, ksize, stride, pad):
        return "frag16" if DENSE == "frag16" and cin % 64 == 0 else "frag3x3"
    if DENSE in ("auto", "dma", "wino"):
        return "dma"
    # streamed weights pay off once a launch has enough steps to amortise the deeper prologue:
    # stride-2 3x3 (72 steps) -12 %, fused head (32) -5 %, 1x1 deblock (8) +8 % -> LDS-staged
    if DENSE == "bstream" or (DENSE == "stream" and conv and ksize * ksize * cin // 16 >= 24):
        return "bstream"
    return "f16x3"                                # "frag" / "frag16" (and any other value): only the 3x3 layers stream


def dense_pack(kind, w_packed, scale=None):
    """Packed f32 weights [Cout,taps,Cin] + folded-BN scale -> (weights in structure `kind`'s format, the scale to hand it:
    the f16x3 split folds its weight exponent into it)."""
    return DENSE_KINDS[kind].pack(w_packed, scale)


def pack_dense(w_packed, scale=None, ksize=None, stride=None, pad=None):
    """dense_pack for the structure the layer takes under MATH / DENSE (``ksize="deconv"`` for the 2x2 transposed conv;
    no geometry: the plain format of MATH)."""
    return dense_pack(dense_structure(w_packed.shape[0], w_packed.shape[2], ksize, stride, pad), w_packed, scale)


_PLAIN_KIND = {torch.float32: "f32", torch.bfloat16: "bf16x6", torch.float16: "f16x3"}


def dense_kind(w_packed):
    """Kind of a weight object: F16x3Packed, or a plain tensor of one of the three dtypes."""
    return w_packed.kind if isinstance(w_packed, F16x3Packed) else _PLAIN_KIND[w_packed.dtype]


def gap_fusable(w_packed):
    """The fused-GAP epilogue exists in the generic f16x3 kernels (plain f16 planes or LDS-DMA images: the deblock
    launches)."""
    return DENSE_KINDS[dense_kind(w_packed)].gap is not None


def dense_launch(who, x, w_packed, scale, shift, geom, relu, out=None, coff=0, gap=None, io=0):
    """The one launch of every structure: out[..., coff:coff+Cout] = conv (geom = (ksize, stride, pad)) or 2x2 transposed
    conv (geom None) of x [B,H,W,Cin], * scale + shift (ReLU).  w_packed, scale: dense_pack's.  out: optional
    [B,OH,OW,ldc] map.  gap: optional [B, parts, ldc] f32 buffer (parts = gap_parts): the launch also writes its
    workgroups' channel sums there (see gap_fusable).  io: IO_* flags (pair pixels)."""
    kind = dense_kind(w_packed)
    row = DENSE_KINDS[kind]
    bev = x if isinstance(x, BevRows) else None
    if bev is not None:
        if geom is None or not neck_rows_ok(kind, bev.index.shape[3], bev.rows.shape[1]):
            raise lib.Al3dError(f"{who}: BevRows input needs the frag3x3 structure under f16x3, two z levels and "
                                f"AL3D_NECK_IN=rows (got {kind!r}); pass x.dense()")
        rows = _dev(bev.rows, torch.float32, "rows")
        if rows.shape[0] == 0:                    # an empty level: every index entry is -1, no row is read
            rows = rows.new_zeros((1, rows.shape[1]))
    else:
        x = _dev(x, torch.float32, "x")
    if isinstance(w_packed, F16x3Packed):
        data, cout, taps, cin = w_packed.data, w_packed.cout, w_packed.taps, w_packed.cin
    else:
        data = _dev(w_packed, w_packed.dtype, "w")
        cout, taps, cin = data.shape[-3:]
    if data.dtype == torch.float16 and scale is None:
        raise lib.Al3dError(f"{who}: f16x3 weights need the scale returned by split_f16x3")
    B, H, W, Cin = x.shape
    fn = row.conv if geom is not None else row.deconv
    ksize, stride, pad = geom if geom is not None else (2, 2, 0)
    if fn is None or cin != Cin or taps != ksize * ksize or not (row.generic or geom == (3, 1, 1)):
        raise lib.Al3dError(f"{who}: {kind!r} weights [Cout={cout}, taps={taps}, Cin={cin}] do not match this layer's geometry")
    if io & ~row.io:
        raise lib.Al3dError(f"{who}: io={io}: the {kind!r} kernel " + (
            "takes the in / out pair-pixel bits only" if row.io & IO_IN_PAIR else
            "reads f32 pixels and writes " + ("f32 or pair pixels" if row.io else "f32 pixels")))
    if gap is not None and row.gap is None:
        raise lib.Al3dError(f"{who}: {kind!r} weights have no fused GAP (see gap_fusable)")
    OH, OW = (2 * H, 2 * W) if geom is None else ((H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1)
    if out is None:
        out = torch.empty((B, OH, OW, cout), dtype=torch.float32, device=x.device)
    assert out.shape[:3] == (B, OH, OW) and out.is_contiguous()
    tail = ()
    if row.gap == "arg" or gap is not None:
        tail += (_ptr(gap), 0 if gap is None else gap.shape[1])
    if row.io:
        tail += (io,)
    if bev is not None:
        lib.call("al3d_conv3x3_nhwc_f16x3_frag_rows", _ptr(rows), rows.shape[1], _ptr(_dev(bev.index, torch.int32, "index")),
                 _ptr(data), _ptr(scale), _ptr(shift), _ptr(out), B, H, W, Cin, cout, out.shape[3], coff, 1 if relu else 0,
                 io, _stream())
        return out
    lib.call(fn + ("_gap" if gap is not None and row.gap == "entry" else ""), _ptr(x), _ptr(data), _ptr(scale), _ptr(shift),
             _ptr(out), B, H, W, Cin, cout, *(geom if row.generic and geom is not None else ()), out.shape[3], coff,
             1 if relu else 0, *tail, _stream())
    return out


def conv2d_nhwc(x, w_packed, scale, shift, ksize, stride, pad, relu, out=None, coff=0, gap=None, io=0):
    return dense_launch("conv2d_nhwc", x, w_packed, scale, shift, (ksize, stride, pad), relu, out, coff, gap, io)


def deconv2x2_nhwc(x, w_packed, scale, shift, relu, out=None, coff=0, gap=None, io=0):
    return dense_launch("deconv2x2_nhwc", x, w_packed, scale, shift, None, relu, out, coff, gap, io)


# ------------------------------------------------------------------ camera-only BEV decoder (csrc/conv2d_res.hip)
# conv2 + bn2 + shortcut + ReLU of the BEV decoder's BasicBlocks under f16x3: "fused" = one launch of
# al3d_conv3x3_res_nhwc_f16x3, "two-step" = the dense dispatch's convolution, then al3d_add_relu_nhwc_f32 (the same
# arithmetic class; the same bits where the dispatch picks the LDS-DMA kernel).  Default two-step: measured 1.8-2.4 x faster
# per layer and 1.3 x on the whole decoder (profiles/camera_decoder.txt); the fused launch is opt-in
RES = _os.environ.get("AL3D_RES", "two-step")
if RES not in ("fused", "two-step"):
    raise lib.Al3dError(f"AL3D_RES={RES!r}: expected fused or two-step")


def pack_res3x3(w_packed, scale=None):
    """Packed f32 weights [Cout,9,Cin] + folded-BN scale -> (weights, scale) for ``conv3x3_res_nhwc`` under MATH: the
    LDS-DMA images of the f16x3 split (``pack_dma_f16x3``), the plain format of the other arithmetics."""
    if MATH == "f16x3":
        return dense_pack("dma", w_packed, scale)
    return dense_pack(MATH, w_packed, scale)


def add_relu_nhwc(x, res, relu=True, out=None):
    """relu(x + res[..., :C]) on channels-last maps (``al3d_add_relu_nhwc_f32``); res may be wider than x; out: an
    optional [..., >= C] map whose first C channels are written (may be x)."""
    x, res = _dev(x, torch.float32, "x"), _dev(res, torch.float32, "res")
    C = x.shape[-1]
    if tuple(res.shape[:-1]) != tuple(x.shape[:-1]):
        raise lib.Al3dError(f"add_relu_nhwc: map sizes {tuple(x.shape)} / {tuple(res.shape)} do not match")
    if out is None:
        out = torch.empty_like(x)
    assert out.shape[:-1] == x.shape[:-1] and out.is_contiguous() and out.dtype == torch.float32
    lib.call("al3d_add_relu_nhwc_f32", _ptr(x), _ptr(res), _ptr(out), x.numel() // max(C, 1), C, C, res.shape[-1],
             out.shape[-1], 1 if relu else 0, _stream())
    return out


def conv3x3_res_nhwc(x, w_packed, scale, shift, res, relu=True, out=None, coff=0):
    """out[..., coff:coff+Cout] = relu((conv3x3/s1/p1(x) * scale + shift) + res[..., :Cout]): conv2 + bn2 + shortcut + ReLU
    of a ResNet BasicBlock.  w_packed, scale: ``pack_res3x3``'s.  f16x3 (LDS-DMA weight images): ONE launch of
    ``al3d_conv3x3_res_nhwc_f16x3``; the other arithmetics: their convolution, then ``al3d_add_relu_nhwc_f32`` (the same
    bits as the fused launch gives on the f16x3 weights).  A geometry the kernels do not serve raises ``Al3dError``."""
    x = _dev(x, torch.float32, "x")
    kind = dense_kind(w_packed)
    B, H, W, Cin = x.shape
    if res is not None:
        res = _dev(res, torch.float32, "res")
        if tuple(res.shape[:3]) != (B, H, W):
            raise lib.Al3dError(f"conv3x3_res_nhwc: residual {tuple(res.shape)} does not match the map {tuple(x.shape)}")
    if kind == "dma":
        cout = w_packed.cout
        if w_packed.taps != 9 or w_packed.cin != Cin:
            raise lib.Al3dError(f"conv3x3_res_nhwc: weights [Cout={cout}, taps={w_packed.taps}, Cin={w_packed.cin}] do not "
                                f"match a 3x3 layer over {Cin} channels")
        if scale is None:
            raise lib.Al3dError("conv3x3_res_nhwc: f16x3 weights need the scale returned by split_f16x3")
        if out is None:
            out = torch.empty((B, H, W, cout), dtype=torch.float32, device=x.device)
        assert out.shape[:3] == (B, H, W) and out.is_contiguous() and out.dtype == torch.float32
        lib.call("al3d_conv3x3_res_nhwc_f16x3", _ptr(x), _ptr(w_packed.data), _ptr(scale), _ptr(shift), _ptr(res), _ptr(out),
                 B, H, W, Cin, cout, 0 if res is None else res.shape[3], out.shape[3], coff, 1 if relu else 0, _stream())
        return out
    if kind not in ("f32", "bf16x6"):
        raise lib.Al3dError(f"conv3x3_res_nhwc: {kind!r} weights; expected pack_res3x3's (LDS-DMA images under f16x3)")
    if res is None:
        raise lib.Al3dError("conv3x3_res_nhwc: null residual")
    y = conv2d_nhwc(x, w_packed, scale, shift, 3, 1, 1, False)
    if out is None:
        return add_relu_nhwc(y, res, relu, out=y)
    if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape[:3]) != (B, H, W):
        raise lib.Al3dError(f"conv3x3_res_nhwc: out must be a contiguous float32 device map [{B},{H},{W},ldc]")
    if coff < 0 or coff % 4 or coff + y.shape[3] > out.shape[3]:
        raise lib.Al3dError(f"conv3x3_res_nhwc: channel window [{coff},{coff + y.shape[3]}) exceeds ldc={out.shape[3]} "
                            "(or coff is not a multiple of 4)")
    lib.call("al3d_add_relu_nhwc_f32", _ptr(y), _ptr(res), out.data_ptr() + 4 * coff, B * H * W, y.shape[3], y.shape[3],
             res.shape[3], out.shape[3], 1 if relu else 0, _stream())
    return out


def upsample_bilinear_ac_nhwc(x, size):
    """Bilinear resize of a channels-last map to ``size`` = (H, W), align_corners=True (``al3d_upsample_bilinear_ac_nhwc_f32``)."""
    x = _dev(x, torch.float32, "x")
    N, h, w, C = x.shape
    H, W = int(size[0]), int(size[1])
    out = torch.empty((N, H, W, C), dtype=torch.float32, device=x.device)
    lib.call("al3d_upsample_bilinear_ac_nhwc_f32", _ptr(x), N, h, w, C, H, W, _ptr(out), _stream())
    return out


def bev_grid_axis(in_scope, out_scope, size):
    """One axis of ``BEVGridTransform`` (heads/segm/vanilla.py:69-75) on the host, in float64 -> (source indices [n, 2]
    int32, weights [n, 2] float32, rounded once).  Output coordinate k: ``v = omin + ostep / 2 + k * ostep``, as many as
    ``torch.arange(omin + ostep / 2, omax, ostep)`` holds (``ceil((omax - start) / ostep)`` in double, ATen's rule);
    ``g = (v - imin) / (imax - imin) * 2 - 1``; source position ``((g + 1) * size - 1) / 2`` (``F.grid_sample``,
    align_corners=False); neighbours ``floor(pos)`` and the next with weights ``(i0 + 1) - pos`` and ``pos - i0``.  An
    index outside [0, size) is stored as -1 with weight 0 (zero padding)."""
    import math

    import numpy as np
    imin, imax = float(in_scope[0]), float(in_scope[1])
    omin, omax, ostep = float(out_scope[0]), float(out_scope[1]), float(out_scope[2])
    start = omin + ostep / 2
    n = max(0, int(math.ceil((omax - start) / ostep)))
    v = start + np.arange(n, dtype=np.float64) * ostep
    g = (v - imin) / (imax - imin) * 2 - 1
    pos = ((g + 1) * size - 1) / 2
    i0 = np.floor(pos)
    idx = np.stack([i0, i0 + 1], axis=1)
    wgt = np.stack([(i0 + 1) - pos, pos - i0], axis=1)
    outside = (idx < 0) | (idx >= size)
    idx[outside], wgt[outside] = -1, 0.0
    return idx.astype(np.int32), wgt.astype(np.float32)


_GRID_TABLES = {}


def bev_grid_tables(input_scope, output_scope, in_hw, device):
    """The four device tables of ``al3d_bev_grid_resample_nhwc_f32`` for a source map of ``in_hw`` = (rows, columns) whose
    rows run along scope 0 and columns along scope 1; kept per device, scopes and size."""
    key = (torch.device(device), tuple(map(tuple, input_scope)), tuple(map(tuple, output_scope)), tuple(in_hw))
    if key not in _GRID_TABLES:
        tabs = []
        for i_s, o_s, size in zip(input_scope, output_scope, in_hw):
            idx, wgt = bev_grid_axis(i_s, o_s, int(size))
            if len(idx) == 0:
                raise lib.Al3dError(f"bev_grid_tables: the output scope {tuple(o_s)} holds no sample")
            tabs += [torch.from_numpy(idx).to(device), torch.from_numpy(wgt).to(device)]
        _GRID_TABLES[key] = tuple(tabs)
    return _GRID_TABLES[key]


def bev_grid_resample_nhwc(x, input_scope, output_scope, out_hw_swapped=False):
    """``BEVGridTransform.forward`` on a channels-last map [N, h, w, C] whose rows run along scope 0 and columns along
    scope 1 -> [N, H, W, C] (``al3d_bev_grid_resample_nhwc_f32``); ``out_hw_swapped``: -> [N, W, H, C], written
    transposed by the same launch."""
    x = _dev(x, torch.float32, "x")
    N, h, w, C = x.shape
    ri, rw, ci, cw = bev_grid_tables(input_scope, output_scope, (h, w), x.device)
    H, W = ri.shape[0], ci.shape[0]
    out = torch.empty((N, W, H, C) if out_hw_swapped else (N, H, W, C), dtype=torch.float32, device=x.device)
    lib.call("al3d_bev_grid_resample_nhwc_f32", _ptr(x), N, h, w, C, _ptr(ri), _ptr(rw), _ptr(ci), _ptr(cw), H, W,
             1 if out_hw_swapped else 0, _ptr(out), _stream())
    return out


def seg_classify(x, weight, bias, with_stats=False):
    """sigmoid(Conv2d(C, K, 1)) of a channels-last map [N, H, W, C] with weight [K, C] and bias [K] -> probabilities
    [N, K, H, W] (``al3d_seg_classify_f32``); ``with_stats``: also (entropy_sum [N, K] float32 -- the binary entropy summed
    over the pixels -- and area [N, K] int32 -- the pixels with p > 0.5)."""
    x, weight, bias = _dev(x, torch.float32, "x"), _dev(weight, torch.float32, "weight"), _dev(bias, torch.float32, "bias")
    N, H, W, C = x.shape
    K = weight.shape[0]
    if tuple(weight.shape) != (K, C) or tuple(bias.shape) != (K,):
        raise lib.Al3dError(f"seg_classify: weight {tuple(weight.shape)} / bias {tuple(bias.shape)} do not match C={C}")
    prob = torch.empty((N, K, H, W), dtype=torch.float32, device=x.device)
    ent = area = ws = None
    if with_stats:
        ent = torch.empty((N, K), dtype=torch.float32, device=x.device)
        area = torch.empty((N, K), dtype=torch.int32, device=x.device)
        ws = torch.empty(max(1, int(lib.load().al3d_seg_classify_workspace_bytes(N, H, W))), dtype=torch.uint8, device=x.device)
    lib.call("al3d_seg_classify_f32", _ptr(x), _ptr(weight), _ptr(bias), N, H, W, C, K, _ptr(prob), _ptr(ent), _ptr(area),
             _ptr(ws), _stream())
    return (prob, ent, area) if with_stats else prob


def gap_parts(OH, OW, deconv):
    return int(lib.load().al3d_gap_parts_count(int(OH), int(OW), 1 if deconv else 0))


def gap_reduce_parts(gap, count):
    """[B, parts, C] workgroup partial sums -> [B, C] means (sum in ascending part order / count)."""
    gap = _dev(gap, torch.float32, "gap")
    B, parts, C = gap.shape
    out = torch.empty((B, C), dtype=torch.float32, device=gap.device)
    lib.call("al3d_gap_reduce_parts_f32", _ptr(gap), B, parts, C, int(count), _ptr(out), _stream())
    return out


# AL3D_GAP=fused (default): the neck's deblock launches emit the embedding's partial sums; "kernel": the stand-alone
# two-stage GAP kernel re-reads the map (round-1 path; W-then-H summation order)
GAP = _os.environ.get("AL3D_GAP", "fused")


def gap_nhwc(x):
    x = _dev(x, torch.float32, "x")
    B, H, W, C = x.shape
    out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    ws = torch.empty((B, H, C), dtype=torch.float32, device=x.device)
    lib.call("al3d_gap_nhwc_f32", _ptr(x), B, H, W, C, _ptr(out), _ptr(ws), _stream())
    return out


def rows_nonfinite(x, out=None):
    """[rows, cols] f32 device rows (row stride may exceed cols) -> uint8 [rows]: 1 where a row holds an inf or NaN."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise lib.Al3dError("rows_nonfinite: expected a [rows, cols] float32 device tensor")
    if x.shape[1] and x.stride(1) != 1:
        x = x.contiguous()
    rows, cols = x.shape
    if out is None:
        out = torch.empty((rows,), dtype=torch.uint8, device=x.device)
    lib.call("al3d_rows_nonfinite_u8", _ptr(x), rows, cols, max(x.stride(0), cols), _ptr(out), _stream())
    return out


# ------------------------------------------------------------------ voxelizer
class Voxelizer:
    """Batched device voxelizer + mean VFE (owns the persistent first-index grid).

    ``cfg`` keys follow the reference's ``voxel_generator`` dict
    (examples/active/cbgs_spatial_temporal.py:279-284): range, voxel_size,
    max_points_in_voxel, max_voxel_num.
    """

    def __init__(self, point_cloud_range, voxel_size, max_points_in_voxel, max_voxel_num,
                 max_batch=8, device="cuda"):
        import ctypes
        import numpy as np
        self.device = torch.device(device)
        rng = np.asarray(point_cloud_range, dtype=np.float32)
        vs = np.asarray(voxel_size, dtype=np.float32)
        # grid_size = round((max - min) / voxel_size) in float32 (voxel_generator.py:11-13)
        grid = np.round((rng[3:] - rng[:3]) / vs).astype(np.int64)
        self.grid_size = grid                      # (x, y, z)
        self.range_min = (ctypes.c_float * 3)(*rng[:3].tolist())
        self.voxel_size = (ctypes.c_float * 3)(*vs.tolist())
        self.grid_c = (ctypes.c_int * 3)(*[int(g) for g in grid])
        self.max_points = int(max_points_in_voxel)
        self.max_voxels = int(max_voxel_num)
        self.max_batch = int(max_batch)
        nbytes = lib.load().al3d_voxelize_grid_bytes(self.max_batch, *[int(g) for g in grid])
        self.grid = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        lib.call("al3d_voxelize_grid_init", _ptr(self.grid), self.max_batch,
                 int(grid[0]), int(grid[1]), int(grid[2]), _stream())

    def __call__(self, points, point_offsets, want_voxels=False):
        """points [P,F] f32 (frames concatenated), point_offsets [B+1] i64 (device).
        Returns dict(feat [M,F], coords [M,4] i32 (b,z,y,x), num_points [M] i32,
        num_voxels [B] i32, voxels [M,max_points,F] | None)."""
        points = _dev(points, torch.float32, "points")
        point_offsets = _dev(point_offsets, torch.int64, "point_offsets")
        B = point_offsets.numel() - 1
        if B > self.max_batch:
            raise lib.Al3dError(f"batch {B} exceeds max_batch {self.max_batch}")
        npts, F = points.shape
        dev = points.device
        rows = B * self.max_voxels
        ws = torch.empty(lib.load().al3d_voxelize_workspace_bytes(npts, B, self.max_voxels),
                         dtype=torch.uint8, device=dev)
        feat = torch.empty((rows, F), dtype=torch.float32, device=dev)
        coords = torch.empty((rows, 4), dtype=torch.int32, device=dev)
        num_points = torch.empty((rows,), dtype=torch.int32, device=dev)
        voxels = torch.empty((rows, self.max_points, F), dtype=torch.float32, device=dev) \
            if want_voxels else None
        num_voxels = torch.empty((B,), dtype=torch.int32, device=dev)
        row_base = torch.empty((B + 1,), dtype=torch.int32, device=dev)
        lib.call("al3d_voxelize_mean_f32", _ptr(points), _ptr(point_offsets), npts, B, F,
                 self.range_min, self.voxel_size, self.grid_c, self.max_points, self.max_voxels,
                 _ptr(self.grid), _ptr(ws), _ptr(feat), _ptr(coords), _ptr(num_points), _ptr(voxels),
                 _ptr(num_voxels), _ptr(row_base), _stream())
        m = int(row_base[-1].item())            # one small D2H per batch
        return dict(feat=feat[:m], coords=coords[:m], num_points=num_points[:m],
                    num_voxels=num_voxels, row_base=row_base, voxel_cap=self.max_voxels,
                    voxels=None if voxels is None else voxels[:m])


_DYN_REDUCE = {"sum": 0, "mean": 1, "max": 2}
_DYN_ORDER = {"zyx": 0, "xyz": 1}


def _dyn_status(status, who):
    """Raise on the status word of the dynamic kernels (a host value: it came with the batch's one D2H)."""
    st = int(status)
    if st & 1:
        raise lib.Al3dError(f"{who}: more voxels than rows_cap")
    if st & 2:
        raise lib.Al3dError(f"{who}: a coordinate lies beyond the stated extents")


class DynamicVoxelizer:
    """Batched dynamic voxelizer (csrc/voxelize_dyn.hip): every in-range point takes part, no cap per voxel or per frame,
    no resident grid -- the scratch is one presence bit per cell per frame plus arrays per point, allocated per call.

    Voxels of a frame come in ascending order of the coordinate triple named by ``order`` ("zyx": this project's encoder
    rows (b, z, y, x); "xyz": the reference's unique_dim order, rows (b, x, y, z)); ``reduce`` is "mean", "sum" or "max"
    over all points of the voxel (ops/voxel/scatter_points.py:73-75 uses mean or max)."""

    def __init__(self, point_cloud_range, voxel_size, reduce="mean", order="zyx", device="cuda"):
        import ctypes
        import numpy as np
        if reduce not in _DYN_REDUCE or order not in _DYN_ORDER:
            raise ValueError(f"reduce must be one of {sorted(_DYN_REDUCE)}, order one of {sorted(_DYN_ORDER)}")
        self.device = torch.device(device)
        rng = np.asarray(point_cloud_range, dtype=np.float32)
        vs = np.asarray(voxel_size, dtype=np.float32)
        grid = np.round((rng[3:] - rng[:3]) / vs).astype(np.int64)
        self.grid_size = grid                      # (x, y, z)
        self.range_min = (ctypes.c_float * 3)(*rng[:3].tolist())
        self.voxel_size = (ctypes.c_float * 3)(*vs.tolist())
        self.grid_c = (ctypes.c_int * 3)(*[int(g) for g in grid])
        self.reduce, self.order = reduce, order

    def workspace_bytes(self, npts, B):
        return lib.load().al3d_voxelize_dynamic_workspace_bytes(int(npts), int(B), *[int(g) for g in self.grid_size])

    def __call__(self, points, point_offsets, want_voxels=False, want_point_coords=False, rows_cap=None):
        """points [P,F] f32 (frames concatenated), point_offsets [B+1] i64 (device).  Returns the dictionary of
        ``Voxelizer.__call__`` (``num_points``: unclipped counts; ``voxel_cap``: the largest per-frame voxel count) plus
        ``point2voxel [P]`` i32 (row or -1) and, on request, ``point_coords [P,3]`` i32 (x, y, z) or -1."""
        if want_voxels:
            raise NotImplementedError("dynamic voxelization has no padded point slots; the dynamic pillar net "
                                      "(DynamicPillarFeatureNet) reads points and point2voxel instead")
        points = _dev(points, torch.float32, "points")
        point_offsets = _dev(point_offsets, torch.int64, "point_offsets")
        B = point_offsets.numel() - 1
        npts, F = points.shape
        dev = points.device
        if npts == 0:                               # nothing to launch on (an empty tensor has no address)
            out = dict(feat=points.new_empty((0, F)), coords=torch.empty((0, 4), dtype=torch.int32, device=dev),
                       num_points=torch.empty((0,), dtype=torch.int32, device=dev),
                       num_voxels=torch.zeros((B,), dtype=torch.int32, device=dev),
                       row_base=torch.zeros((B + 1,), dtype=torch.int32, device=dev), voxel_cap=1, voxels=None,
                       point2voxel=torch.empty((0,), dtype=torch.int32, device=dev))
            if want_point_coords:
                out["point_coords"] = torch.empty((0, 3), dtype=torch.int32, device=dev)
            return out
        rows = npts if rows_cap is None else int(rows_cap)
        ws = torch.empty(max(self.workspace_bytes(npts, B), 1), dtype=torch.uint8, device=dev)
        feat = torch.empty((rows, F), dtype=torch.float32, device=dev)
        coords = torch.empty((rows, 4), dtype=torch.int32, device=dev)
        counts = torch.empty((rows,), dtype=torch.int32, device=dev)
        pcoords = torch.empty((npts, 3), dtype=torch.int32, device=dev) if want_point_coords else None
        p2v = torch.empty((npts,), dtype=torch.int32, device=dev)
        num_voxels = torch.empty((B,), dtype=torch.int32, device=dev)
        # row_base [B+1] and the status word share one tensor: one D2H per batch
        tail = torch.empty((B + 2,), dtype=torch.int32, device=dev)
        lib.call("al3d_voxelize_dynamic_f32", _ptr(points), _ptr(point_offsets), npts, B, F, self.range_min,
                 self.voxel_size, self.grid_c, _DYN_ORDER[self.order], _DYN_REDUCE[self.reduce], rows, _ptr(ws),
                 _ptr(feat), _ptr(coords), _ptr(counts), _ptr(pcoords), _ptr(p2v), _ptr(num_voxels), _ptr(tail),
                 tail.data_ptr() + 4 * (B + 1), _stream())
        host = tail.cpu()
        _dyn_status(host[B + 1], "al3d_voxelize_dynamic_f32")
        m = int(host[B])
        cap = int((host[1:B + 1] - host[:B]).max()) if B > 0 else 0
        out = dict(feat=feat[:m], coords=coords[:m], num_points=counts[:m], num_voxels=num_voxels,
                   row_base=tail[:B + 1], voxel_cap=max(cap, 1), voxels=None, point2voxel=p2v)
        if want_point_coords:
            out["point_coords"] = pcoords
        return out


def dynamic_scatter_rows(feats, coors, reduce="max"):
    """``dynamic_scatter`` on given coordinates (ops/voxel/scatter_points.py:8-50): feats [N,C] f32, coors [N,3] int; rows
    with a negative coordinate are dropped.  Returns (voxel_feats [M,C], voxel_coors [M,3] i32 sorted ascending,
    point2voxel [N] i32, counts [M] i32)."""
    import ctypes
    feats = _dev(feats, torch.float32, "feats")
    coors = _dev(coors.to(torch.int32), torch.int32, "coors")
    if coors.dim() != 2 or coors.shape[1] != 3 or coors.shape[0] != feats.shape[0]:
        raise ValueError("coors must be [N, 3] with one row per feature row")
    if reduce not in _DYN_REDUCE:
        raise ValueError(f"reduce_type must be one of {sorted(_DYN_REDUCE)}")
    n, C = feats.shape
    dev = feats.device
    if n == 0:                                      # scatter_points_cuda.cu:192-196
        empty = torch.empty((0,), dtype=torch.int32, device=dev)
        return feats.new_empty((0, C)), torch.empty((0, 3), dtype=torch.int32, device=dev), empty, empty
    ext = [max(int(v) + 1, 1) for v in coors.max(dim=0).values.tolist()]
    dims = (ctypes.c_int * 3)(*ext)
    ws = torch.empty(max(lib.load().al3d_voxelize_dynamic_workspace_bytes(n, 1, *ext), 1), dtype=torch.uint8, device=dev)
    out = torch.empty((n, C), dtype=torch.float32, device=dev)
    ocoors = torch.empty((n, 3), dtype=torch.int32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    p2v = torch.empty((n,), dtype=torch.int32, device=dev)
    tail = torch.empty((2,), dtype=torch.int32, device=dev)        # num_voxels, status
    lib.call("al3d_dynamic_scatter_f32", _ptr(feats), _ptr(coors), n, C, dims, _DYN_REDUCE[reduce], n, _ptr(ws),
             _ptr(out), _ptr(ocoors), _ptr(counts), _ptr(p2v), _ptr(tail), tail.data_ptr() + 4, _stream())
    host = tail.cpu()
    _dyn_status(host[1], "al3d_dynamic_scatter_f32")
    m = int(host[0])
    return out[:m], ocoors[:m], p2v, counts[:m]


def voxelizer_class(voxel_cfg):
    """The voxelizer class a ``voxel_generator`` dict selects (pure: builds nothing): the dynamic one iff
    ``max_points_in_voxel == -1`` or ``max_voxel_num == -1`` (ops/voxel/voxelize.py:47)."""
    dynamic = int(voxel_cfg["max_points_in_voxel"]) == -1 or int(voxel_cfg["max_voxel_num"]) == -1
    return DynamicVoxelizer if dynamic else Voxelizer


def build_voxelizer(voxel_cfg, max_batch, device, with_points=False):
    """The voxelizer of a ``voxel_generator`` dict, for the loaders and the pipeline stage."""
    if voxelizer_class(voxel_cfg) is DynamicVoxelizer:
        if with_points:
            raise NotImplementedError("with_points=True (PillarFeatureNet) needs the padded point slots of the hard "
                                      "voxelizer -- set max_points_in_voxel and max_voxel_num, or use the dynamic pillar "
                                      "net (DynamicPillarFeatureNet) and build the loader with keep_points=True")
        return DynamicVoxelizer(voxel_cfg["range"], voxel_cfg["voxel_size"], reduce="mean", order="zyx", device=device)
    return Voxelizer(voxel_cfg["range"], voxel_cfg["voxel_size"], voxel_cfg["max_points_in_voxel"],
                     voxel_cfg["max_voxel_num"], max_batch=max_batch, device=device)


# ------------------------------------------------------------------ PointPillars pillar net
class PillarNet:
    """Folded PFN layers of a ``PillarFeatureNet`` for ``al3d_pillar_net_*`` (csrc/pillars.hip).  ``layers``: one or
    two ``(linear, bn)`` pairs in eval mode; weights are transposed to [in, units] and BN folded to scale / shift."""

    def __init__(self, layers, vx, vy, x_offset, y_offset, with_distance, device):
        if not 1 <= len(layers) <= 2:
            raise lib.Al3dError(f"PillarNet: 1 or 2 PFN layers supported, got {len(layers)}")
        self.packs = []
        for lin, bn in layers:
            units = lin.weight.shape[0]
            if units % 16 or not 16 <= units <= 128:
                raise lib.Al3dError(f"PillarNet: a PFN layer has {units} units; the kernel needs a multiple of 16 "
                                    "in [16, 128]")
            scale, shift = fold_bn(bn)
            w = lin.weight.detach().float().t().contiguous()
            self.packs.append((w.to(device), scale.to(device), shift.to(device), units))
        self.geom = (float(vx), float(vy), float(x_offset), float(y_offset), int(bool(with_distance)))
        self.channels = self.packs[-1][3]
        self._status = None                         # device status word of the dynamic calls, allocated on first use

    def _args(self, voxels, num_points, coords):
        voxels = _dev(voxels, torch.float32, "voxels").contiguous()
        num_points = _dev(num_points.to(torch.int32), torch.int32, "num_points").contiguous()
        coords = _dev(coords.to(torch.int32), torch.int32, "coords").contiguous()
        M, P, F = voxels.shape
        if num_points.numel() != M or tuple(coords.shape) != (M, 4):
            raise lib.Al3dError(f"PillarNet: {M} pillars but num_points {tuple(num_points.shape)}, "
                                f"coords {tuple(coords.shape)}")
        w1, s1, b1, u1 = self.packs[0]
        if w1.shape[0] != F + 5 + self.geom[4]:
            raise lib.Al3dError(f"PillarNet: {F} point features need a first layer of {F + 5 + self.geom[4]} inputs, "
                                f"got {w1.shape[0]}")
        w2, s2, b2, u2 = self.packs[1] if len(self.packs) == 2 else (None, None, None, 0)
        keep = (voxels, num_points, coords)        # the pointers below stay valid while the caller holds these
        return (_ptr(voxels), _ptr(num_points), _ptr(coords), M, P, F, *self.geom,
                _ptr(w1), _ptr(s1), _ptr(b1), u1, _ptr(w2), _ptr(s2), _ptr(b2), u2), keep

    def rows(self, voxels, num_points, coords):
        """-> [M, C] pillar features (PillarFeatureNet.forward)."""
        args, keep = self._args(voxels, num_points, coords)
        out = torch.empty((args[3], self.channels), dtype=torch.float32, device=keep[0].device)
        lib.call("al3d_pillar_net_f32", *args, _ptr(out), _stream())
        return out

    def canvas(self, voxels, num_points, coords, batch, ny, nx):
        """-> NHWC canvas [batch, ny, nx, C]: the net fused with the scatter (zero where there is no pillar)."""
        args, keep = self._args(voxels, num_points, coords)
        out = torch.empty((batch, ny, nx, self.channels), dtype=torch.float32, device=keep[0].device)
        lib.call("al3d_pillar_net_scatter_f32", *args, batch, ny, nx, _ptr(out), _stream())
        return out

    # ---- all points of every pillar (csrc/pillars_dyn.hip): the dynamic voxelizer's output, no padded slots
    def _dynamic(self, points, point2voxel, mean, coords, batch, ny, nx, canvas, check, chunk_points=0, max_blocks=0):
        points = _dev(points, torch.float32, "points").contiguous()
        point2voxel = _dev(point2voxel.to(torch.int32), torch.int32, "point2voxel").contiguous()
        mean = _dev(mean, torch.float32, "mean")
        if mean.dim() != 2 or mean.shape[1] < 3:
            raise lib.Al3dError(f"PillarNet: mean {tuple(mean.shape)}: need [M, >= 3] rows of the pillar means")
        if mean.shape[0] <= 1 or mean.stride(1) != 1:       # a row slice of the voxelizer's buffer is read in place
            mean = mean.contiguous()
        coords = _dev(coords.to(torch.int32), torch.int32, "coords").contiguous()
        npts, F = points.shape
        M = mean.shape[0]
        if point2voxel.numel() != npts or tuple(coords.shape) != (M, 4):
            raise lib.Al3dError(f"PillarNet: {npts} points but point2voxel {tuple(point2voxel.shape)}; {M} pillars but "
                                f"coords {tuple(coords.shape)}")
        w1, s1, b1, u1 = self.packs[0]
        if w1.shape[0] != F + 5 + self.geom[4]:
            raise lib.Al3dError(f"PillarNet: {F} point features need a first layer of {F + 5 + self.geom[4]} inputs, "
                                f"got {w1.shape[0]}")
        two = len(self.packs) == 2
        w2, s2, b2, u2 = self.packs[1] if two else (None, None, None, 0)
        dev = points.device
        shape = (batch, ny, nx, self.channels) if canvas else (M, self.channels)
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        ws = torch.empty(max(lib.load().al3d_pillar_net_dynamic_workspace_bytes(M, u1, int(two)), 1), dtype=torch.uint8,
                         device=dev)
        if self._status is None or self._status.device != dev:
            self._status = torch.zeros((1,), dtype=torch.int32, device=dev)
        ld = int(mean.stride(0)) if M > 1 else int(mean.shape[1])
        lib.call("al3d_pillar_net_dynamic_launch_f32", _ptr(points), _ptr(point2voxel), npts, F, _ptr(mean), ld,
                 _ptr(coords), M, *self.geom, _ptr(w1), _ptr(s1), _ptr(b1), u1, _ptr(w2), _ptr(s2), _ptr(b2), u2,
                 batch, ny, nx, _ptr(out), int(canvas), _ptr(ws), _ptr(self._status), int(chunk_points), int(max_blocks),
                 _stream())
        if check:
            self.dynamic_status()
        return out

    def dynamic_status(self):
        """Read (one D2H) and clear the status word of the dynamic calls; raises when a point2voxel value lay outside
        [-1, M).  The sweep does not call it: a loader's ``point2voxel`` comes from the dynamic voxelizer, whose own status
        word was read with that batch's host sync."""
        if self._status is None:
            return
        st = int(self._status.item())
        if st:
            self._status.zero_()
            raise lib.Al3dError("al3d_pillar_net_dynamic_f32: a point2voxel value lies outside [-1, M) (point skipped)")

    def rows_dynamic(self, points, point2voxel, mean, coords, check=True, **shape):
        """-> [M, C] pillar features over all points: points [N, F], point2voxel [N] (row or -1), mean [M, >= 3] (the
        dynamic voxelizer's ``feat``), coords [M, 4] (b, z, y, x).  No padded-slot row takes part in the max."""
        return self._dynamic(points, point2voxel, mean, coords, 0, 1, 1, False, check, **shape)

    def canvas_dynamic(self, points, point2voxel, mean, coords, batch, ny, nx, check=True, **shape):
        """-> NHWC canvas [batch, ny, nx, C]: ``rows_dynamic`` fused with the scatter (zero where there is no pillar)."""
        return self._dynamic(points, point2voxel, mean, coords, int(batch), int(ny), int(nx), True, check, **shape)


# ------------------------------------------------------------------ fused VFE reader
class VfeNet:
    """Folded layers of a ``VoxelFeatureExtractor`` / ``VoxelFeatureExtractorV2`` for ``al3d_vfe_net_*`` (csrc/vfe.hip).
    ``layers``: ``(linear, norm)`` pairs in eval mode, the one or two VFE layers first and the final linear last; a norm
    without running statistics (``use_norm=False``) folds to scale 1, shift ``linear.bias``.  Weights are transposed to
    [in, units]."""

    def __init__(self, layers, with_distance, device):
        if not 2 <= len(layers) <= 3:
            raise lib.Al3dError(f"VfeNet: 1 or 2 VFE layers + the final linear supported, got {len(layers)} layers")
        self.packs = []
        for lin, bn in layers:
            units = lin.weight.shape[0]
            if isinstance(bn, torch.nn.BatchNorm1d):
                scale, shift = fold_bn(bn, lin.bias)
            else:
                scale = torch.ones(units, dtype=torch.float32)
                shift = (lin.bias.detach().float().cpu() if lin.bias is not None else torch.zeros(units)).contiguous()
            w = lin.weight.detach().float().t().contiguous()
            self.packs.append((w.to(device), scale.to(device), shift.to(device), units))
        for _, _, _, units in self.packs[:-1]:
            if units % 16 or not 16 <= units <= 64:
                raise lib.Al3dError(f"VfeNet: a VFE layer has {units} units; the kernel needs a multiple of 16 in [16, 64]")
        self.with_distance = int(bool(with_distance))
        self.channels = self.packs[-1][3]
        if self.channels != 2 * self.packs[-2][3]:
            raise lib.Al3dError(f"VfeNet: the final linear has {self.channels} units, the last VFE layer gives "
                                f"{2 * self.packs[-2][3]}")

    def rows(self, voxels, num_points, voxels_per_wave=None, max_blocks=None):
        """-> [M, C] voxel features; ``voxels_per_wave`` / ``max_blocks`` state the launch shape (same bits)."""
        voxels = _dev(voxels, torch.float32, "voxels").contiguous()
        num_points = _dev(num_points.to(torch.int32), torch.int32, "num_points").contiguous()
        if voxels.dim() != 3 or num_points.numel() != voxels.shape[0]:
            raise lib.Al3dError(f"VfeNet: voxels {tuple(voxels.shape)} (need [M, T, F]), num_points "
                                f"{tuple(num_points.shape)}")
        M, T, F = voxels.shape
        w1, s1, b1, u1 = self.packs[0]
        if w1.shape[0] != F + 3 + self.with_distance:
            raise lib.Al3dError(f"VfeNet: {F} point features need a first layer of {F + 3 + self.with_distance} inputs, "
                                f"got {w1.shape[0]}")
        w2, s2, b2, u2 = self.packs[1] if len(self.packs) == 3 else (None, None, None, 0)
        w3, s3, b3, c = self.packs[-1]
        out = torch.empty((M, c), dtype=torch.float32, device=voxels.device)
        args = (_ptr(voxels), _ptr(num_points), M, T, F, self.with_distance, _ptr(w1), _ptr(s1), _ptr(b1), u1,
                _ptr(w2), _ptr(s2), _ptr(b2), u2, _ptr(w3), _ptr(s3), _ptr(b3), c, _ptr(out))
        if voxels_per_wave is None and max_blocks is None:
            lib.call("al3d_vfe_net_f32", *args, _stream())
        else:
            lib.call("al3d_vfe_net_launch_f32", *args, int(voxels_per_wave or 0), int(max_blocks or 0), _stream())
        return out


def pillar_scatter(rows, coords, batch, ny, nx):
    """PointPillarsScatter: rows [M, C] at coords (b, z, y, x) -> NHWC canvas [batch, ny, nx, C], zero elsewhere."""
    rows = _dev(rows, torch.float32, "rows").contiguous()
    coords = _dev(coords.to(torch.int32), torch.int32, "coords").contiguous()
    M, C = rows.shape
    out = torch.empty((batch, ny, nx, C), dtype=torch.float32, device=rows.device)
    lib.call("al3d_pillar_scatter_nhwc_f32", _ptr(rows), _ptr(coords), M, C, batch, ny, nx, _ptr(out), _stream())
    return out


# ------------------------------------------------------------------ single sparse conv layer
def sparse_conv_layer(feats, coords, batch, in_shape, weight, ksize, stride, pad, subm,
                      scale=None, shift=None, residual=None, relu=False, mfma=None, io=0):
    """One spconv layer on device through the encoder's dispatch (used by the tests).  mfma: a SPARSE structure, by
    default the one the encoder would run on rows in the caller's order.  feats [n,Cin] f32, coords [n,4] i32 (b,z,y,x),
    weight [kz,ky,kx,Cin,Cout].  Returns (fout [n_out,Cout], coords_out [n_out,4] (strided: raster order), out_shape)."""
    dev = feats.device
    k = [int(v) for v in ksize]
    n, cin = feats.shape
    cout = weight.shape[-1]
    K = k[0] * k[1] * k[2]
    name, width = (mfma, cin) if mfma is not None else sparse_structure(cin, cout, K, subm, False)[:2]
    if width != cin:
        feats = torch.nn.functional.pad(feats, (0, width - cin))
    w, scale = sparse_pack(name, weight.reshape(K, cin, cout).float(), scale, width)
    tiled = SPARSE[name][2]
    dims = [int(v) for v in in_shape]
    grid_in = torch.full((batch * dims[0] * dims[1] * dims[2],), -1, dtype=torch.int32, device=dev)
    lib.call("al3d_sp_scatter_index", _ptr(coords), n, batch, *dims, _ptr(grid_in), 1, _stream())
    if subm:
        ocoords, oshape = coords, dims
        tab = sparse_table(tiled, coords, n, batch, dims, grid_in, k)
    else:
        s3, p3 = [int(v) for v in stride], [int(v) for v in pad]
        oshape = [(dims[d] + 2 * p3[d] - k[d]) // s3[d] + 1 for d in range(3)]
        grid_out = torch.full((batch * oshape[0] * oshape[1] * oshape[2],), -1, dtype=torch.int32, device=dev)
        ocoords = sparse_down_sites(coords, n, k, s3, p3, batch, oshape, grid_out)
        tab = sparse_table(tiled, ocoords, ocoords.shape[0], batch, dims, grid_in, k, s3, p3)
    sparse_side(name, tab, width, cout)
    if "plan" in tab:
        sparse_conv_layer.last_plan = tab["plan"]
    out = torch.empty((tab["n"], cout), dtype=torch.float32, device=dev)
    sparse_launch(name, feats, tab, w, width, cout, scale, shift, residual, relu, out, io)
    return out, ocoords, oshape


def box_decode(enc, anchors):
    enc = _dev(enc, torch.float32, "enc").reshape(-1, 10)
    anchors = _dev(anchors, torch.float32, "anchors").reshape(-1, 9)
    out = torch.empty((enc.shape[0], 9), dtype=torch.float32, device=enc.device)
    lib.call("al3d_box_decode_f32", _ptr(enc), _ptr(anchors), enc.shape[0], _ptr(out), _stream())
    return out


# ------------------------------------------------------------------ CenterPoint head (csrc/center_head.hip)
def conv3x3_grouped_nhwc(x, w, bias, cout, coff, out=None, ldc=None):
    """The last convolutions of separate heads in one launch: x [B,H,W,G*64]; group g convolves its own 64 channels
    with w rows [sum(cout[:g]) : sum(cout[:g+1])] of w [sum cout, 9, 64] (3x3, padding 1, tap = ky*3+kx) plus bias and
    writes cout[g] <= 8 channels at coff[g] of out [B,H,W,ldc]."""
    import ctypes
    x = _dev(x, torch.float32, "x")
    w = _dev(w, torch.float32, "w")
    bias = _dev(bias, torch.float32, "bias")
    B, H, W, C = x.shape
    G = len(cout)
    if C != G * 64 or tuple(w.shape) != (sum(cout), 9, 64) or bias.numel() != sum(cout) or len(coff) != G:
        raise lib.Al3dError("conv3x3_grouped_nhwc: x must hold 64 channels per group, w [sum cout, 9, 64], bias [sum cout]")
    if out is None:
        ldc = max(o + c for o, c in zip(coff, cout)) if ldc is None else ldc
        out = torch.empty((B, H, W, ldc), dtype=torch.float32, device=x.device)
    assert out.shape[:3] == (B, H, W) and out.is_contiguous() and out.dtype == torch.float32
    IntG = ctypes.c_int * G
    lib.call("al3d_conv3x3_grouped_nhwc_f32", _ptr(x), _ptr(w), _ptr(bias), _ptr(out), B, H, W, G,
             IntG(*[int(c) for c in cout]), IntG(*[int(c) for c in coff]), out.shape[3], _stream())
    return out


CENTER_CHANNELS = ("heatmap", "reg", "height", "dim", "rot", "vel")      # order of a task's row in ``chan_off``


def center_decode_nms(hout, task_ncls, chan_off, *, swapped, max_num, norm_bbox, out_size_factor, voxel_size, pc_range,
                      coder_score_threshold, post_center_range, nms_type, nms_scale, min_radius, score_threshold, nms_thr,
                      pre_max_size, post_max_size, post_center_limit_range, merge=True):
    """CenterPoint post-processing of a head output ``hout`` [B,D0,D1,CH] (channels-last, raw) in one device call
    (``al3d_center_decode_nms_f32``; semantics in include/al3d.h).  ``chan_off[t]``: channels of CENTER_CHANNELS for
    task t (reg / vel: -1 when the head has none).  ``nms_type``: "rotate" / "circle" or one per task; ``nms_scale``:
    per task, per class.  A falsy ``coder_score_threshold`` / non-positive ``score_threshold`` filters nothing, as in
    the reference.  -> boxes [B,nt,post,9], scores [B,nt,post], labels i32 [B,nt,post], counts i32 [B,nt] on the
    device; nothing is read back."""
    import ctypes
    hout = _dev(hout, torch.float32, "hout")
    B, D0, D1, CH = hout.shape
    nt = len(task_ncls)
    kinds = [nms_type] * nt if isinstance(nms_type, str) else list(nms_type)
    if len(kinds) != nt or any(k not in ("rotate", "circle") for k in kinds):
        raise NotImplementedError(f"nms_type {nms_type!r}: one of 'rotate' / 'circle', or one per task")
    if int(max_num) > D0 * D1:
        raise lib.Al3dError(f"center_decode_nms: max_num {max_num} exceeds the {D0} x {D1} cells of the map (torch.topk raises too)")
    post = int(post_max_size)
    dev = hout.device
    boxes = torch.empty((B, nt, post, 9), dtype=torch.float32, device=dev)
    scores = torch.empty((B, nt, post), dtype=torch.float32, device=dev)
    labels = torch.empty((B, nt, post), dtype=torch.int32, device=dev)
    counts = torch.zeros((B, nt), dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.load().al3d_center_decode_nms_workspace_bytes(B, D0, D1, sum(task_ncls))), 1),
                     dtype=torch.uint8, device=dev)
    IntT, F6 = ctypes.c_int * nt, ctypes.c_float * 6
    scale = [1.0] * (4 * nt)
    for t in range(nt):
        for c in range(min(task_ncls[t], 4)):          # a fifth class is the library's to refuse, not an IndexError here
            scale[4 * t + c] = float(nms_scale[t][c])
    radius = [float(min_radius[t]) if kinds[t] == "circle" else 0.0 for t in range(nt)]
    limit = None if post_center_limit_range is None or len(post_center_limit_range) == 0 \
        else F6(*[float(v) for v in post_center_limit_range])
    lib.call("al3d_center_decode_nms_f32", _ptr(hout), B, D0, D1, CH, 1 if swapped else 0, nt,
             IntT(*[int(n) for n in task_ncls]), (ctypes.c_int * (6 * nt))(*[int(v) for row in chan_off for v in row]),
             int(max_num), 1 if norm_bbox else 0,
             (ctypes.c_float * 5)(float(out_size_factor), float(voxel_size[0]), float(voxel_size[1]), float(pc_range[0]),
                                  float(pc_range[1])),
             float(coder_score_threshold) if coder_score_threshold else -1.0, F6(*[float(v) for v in post_center_range]),
             IntT(*[0 if k == "rotate" else 1 for k in kinds]), (ctypes.c_float * (4 * nt))(*scale),
             (ctypes.c_float * nt)(*radius), float(score_threshold) if score_threshold and score_threshold > 0.0 else -1.0,
             float(nms_thr), int(pre_max_size), post, limit, 1 if merge else 0, _ptr(boxes), _ptr(scores), _ptr(labels),
             _ptr(counts), _ptr(ws), _stream())
    return boxes, scores, labels, counts


_BOX_CORNERS = (0, 1, 3, 2, 4, 5, 7, 6)        # corners_nd's order of the unit cube's corners (z fastest, then swapped pairs)
_BOX_FACES = ((0, 1, 2, 3), (7, 6, 5, 4), (0, 3, 7, 4), (1, 5, 6, 2), (0, 4, 5, 1), (3, 2, 6, 7))   # normals point inside


def box_planes(boxes):
    """The six inward planes ``(n0, n1, n2, d)`` of every box, ``[R, 6, 4]`` float32, for ``al3d_points_in_boxes_*``.

    Host numpy on purpose: a frame has tens of boxes, and the SAME float32 calls as the reference keep ``sinf`` / ``cosf``
    differences and summation orders out of the membership test -- ``corners_nd`` (box_np_ops.py:269-305),
    ``rotation_3d_in_axis(axis=2)`` with its einsum (:360-396), ``+= centers`` (:474), ``corner_to_surfaces_3d``
    (:1111-1131) and the formulas of ``surface_equ_3d_jitv2`` (geometry.py:380-405).  ``boxes [R, >= 7]`` float32 numpy:
    centre, three sizes, ..., the angle in the LAST column (``points_in_rbbox``, box_np_ops.py:1102-1108)."""
    import numpy as np
    boxes = np.asarray(boxes)
    if boxes.dtype != np.float32 or boxes.ndim != 2 or boxes.shape[1] < 7:
        raise lib.Al3dError(f"box_planes: boxes [R, >= 7] float32 expected, got {boxes.dtype} {boxes.shape}")
    centers, dims, angles = boxes[:, :3], boxes[:, 3:6], boxes[:, -1]
    unit = np.stack(np.unravel_index(np.arange(8), [2, 2, 2]), axis=1).astype(np.float32)[list(_BOX_CORNERS)]
    unit = unit - np.array((0.5, 0.5, 0.5), dtype=np.float32)
    corners = dims.reshape([-1, 1, 3]) * unit.reshape([1, 8, 3])
    s, c = np.sin(angles), np.cos(angles)
    one, zero = np.ones_like(c), np.zeros_like(c)
    rot_t = np.stack([[c, -s, zero], [s, c, zero], [zero, zero, one]])
    corners = np.einsum("aij,jka->aik", corners, rot_t)
    corners += centers.reshape([-1, 1, 3])
    faces = corners[:, np.array(_BOX_FACES)]                      # [R, 6, 4, 3]
    a, b = faces[:, :, 0] - faces[:, :, 1], faces[:, :, 1] - faces[:, :, 2]
    planes = np.empty((boxes.shape[0], 6, 4), dtype=np.float32)
    planes[..., 0] = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    planes[..., 1] = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
    planes[..., 2] = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    p0 = faces[:, :, 0]
    planes[..., 3] = -p0[..., 0] * planes[..., 0] - p0[..., 1] * planes[..., 1] - p0[..., 2] * planes[..., 2]
    return planes


# ---- anchor target assignment (al3d_assign_targets_f32) -----------------------------------------------------------------
class AssignClass(ctypes.Structure):
    """``al3d_assign_class_t`` of include/al3d.h."""
    _fields_ = [("out_base", ctypes.c_int64), ("anchor_begin", ctypes.c_int), ("num_loc", ctypes.c_int),
                ("num_rot", ctypes.c_int), ("slot_offset", ctypes.c_int), ("slot_stride", ctypes.c_int),
                ("task_anchors", ctypes.c_int), ("label", ctypes.c_int), ("matched", ctypes.c_float),
                ("unmatched", ctypes.c_float)]


class AssignPlan:
    """What every frame shares: the anchors grouped by class with their near boxes on the device, and the class table.

    ``tasks``: per task a list of ``dict(class_name, anchors, matched, unmatched)``, the class's anchors
    ``[..., per-location anchors, n_dim]`` float32 numpy in the task's class order (``generate_anchors_dict``,
    target_assigner.py:167-187).  ``anchors_bv`` is ``rbbox2d_to_near_bbox`` on the host (preprocess.py:367-370), once:
    the pi/4 standing-or-lying decision and ``limit_period`` are the reference's own float32 arithmetic."""

    def __init__(self, tasks, box_coder, device):
        import numpy as np
        from .ops.box_np_ops import rbbox2d_to_near_bbox
        self.device = torch.device(device)
        self.n_dim, self.code_size = int(box_coder.n_dim), int(box_coder.code_size)
        self.vec_encode, self.linear_dim, self.norm_velo = bool(box_coder.vec_encode), bool(box_coder.linear_dim), \
            bool(box_coder.norm_velo)
        self.class_names, self.task_of, self.task_anchors, rows, flat = [], [], [], [], []
        begin = 0
        for t, classes in enumerate(tasks):
            stride = sum(int(c["anchors"].shape[-2]) for c in classes)
            slot, num_loc = 0, None
            for k, c in enumerate(classes):
                a = np.ascontiguousarray(c["anchors"], dtype=np.float32)
                if a.shape[-1] != self.n_dim:
                    raise lib.Al3dError(f"assign_targets: class {c['class_name']!r} has {a.shape[-1]}-column anchors, the box "
                                        f"coder's n_dim is {self.n_dim}")
                num_rot = int(a.shape[-2])
                a = a.reshape(-1, num_rot, self.n_dim)
                if num_loc is not None and a.shape[0] != num_loc:
                    raise lib.Al3dError("assign_targets: the classes of one task must share the feature map")
                num_loc = int(a.shape[0])
                rows.append(dict(anchor_begin=begin, num_loc=num_loc, num_rot=num_rot, slot_offset=slot, slot_stride=stride,
                                 task_anchors=num_loc * stride, label=k + 1, matched=float(np.float32(c["matched"])),
                                 unmatched=float(np.float32(c["unmatched"]))))
                flat.append(a.reshape(-1, self.n_dim))
                self.class_names.append(c["class_name"])
                self.task_of.append(t)
                begin += num_loc * num_rot
                slot += num_rot
            self.task_anchors.append((num_loc or 0) * stride)
        self.rows = rows
        anchors = np.concatenate(flat, axis=0) if flat else np.zeros((0, self.n_dim), np.float32)
        self.anchors_np = anchors
        self.anchors_bv_np = np.ascontiguousarray(rbbox2d_to_near_bbox(anchors[:, [0, 1, 3, 4, -1]]), dtype=np.float32)
        self.anchors = torch.from_numpy(anchors).to(self.device)
        self.anchors_bv = torch.from_numpy(self.anchors_bv_np).to(self.device)
        if len(set(self.class_names)) != len(self.class_names):
            raise lib.Al3dError(f"assign_targets: a class name occurs twice in {self.class_names}: boxes are given to classes by name")
        self.class_index = {n: i for i, n in enumerate(self.class_names)}
        self._tables = {}

    def table(self, B):
        """-> (ctypes array of AssignClass for a batch of B frames, out_rows, per-task first row); kept per B."""
        if B in self._tables:
            return self._tables[B]
        base, bases = 0, []
        for n in self.task_anchors:
            bases.append(base)
            base += B * n
        tab = (AssignClass * len(self.rows))()
        for i, r in enumerate(self.rows):
            tab[i] = AssignClass(out_base=bases[self.task_of[i]], **r)
        self._tables[B] = (tab, base, bases)
        return self._tables[B]


def assign_targets(plan, gt_boxes, gt_names=None, gt_class=None, limit_angle=True, launch=None, with_index=True):
    """``al3d_assign_targets_f32`` for a batch: AssignTarget's train branch (preprocess.py:396-479) for every frame and task
    in one launch, nothing read back.

    ``gt_boxes``: per frame ``[n_i, n_dim]`` float32 numpy; ``gt_names``: per frame the boxes' class names (a box whose name
    no class carries is ignored, its row still counts) or ``gt_class``: per frame int indexes into ``plan.class_names``.
    Like the reference the boxes pass ``limit_period(r, 0.5, 2 pi)`` (preprocess.py:413-417, ``limit_angle``) and
    ``np.nan_to_num`` (target_assigner.py:97); their near boxes are the reference's numpy calls on the host.
    -> ``dict(labels, reg_targets, reg_weights, gt_index)``, each a list over tasks of ``[B, A_t]`` (``[B, A_t, code_size]``)
    device tensors, plus ``gt_overlap [R]`` and the host ``gt_off [B + 1]``.  ``launch``: (groups, threads, chunk)."""
    import numpy as np
    from .ops.box_np_ops import limit_period, rbbox2d_to_near_bbox
    B, nd = len(gt_boxes), plan.n_dim
    counts = [int(np.asarray(b).shape[0]) for b in gt_boxes]
    gt_off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(counts, out=gt_off[1:])
    R = int(gt_off[-1])
    boxes = np.zeros((R, nd), dtype=np.float32)
    cls = np.full((R,), -1, dtype=np.int32)
    for b in range(B):
        if counts[b] == 0:
            continue
        g = np.asarray(gt_boxes[b])
        if g.dtype != np.float32 or g.ndim != 2 or g.shape[1] != nd:
            raise lib.Al3dError(f"assign_targets: frame {b}: gt_boxes [n, {nd}] float32 expected, got {g.dtype} {g.shape}")
        boxes[gt_off[b]:gt_off[b + 1]] = g
        if gt_class is not None:
            cls[gt_off[b]:gt_off[b + 1]] = np.asarray(gt_class[b], dtype=np.int32)
        else:
            cls[gt_off[b]:gt_off[b + 1]] = [plan.class_index.get(str(n), -1) for n in gt_names[b]]
    if limit_angle:
        boxes[:, -1] = limit_period(boxes[:, -1], offset=0.5, period=np.pi * 2)
    boxes = np.nan_to_num(boxes)
    bv = np.ascontiguousarray(rbbox2d_to_near_bbox(boxes[:, [0, 1, 3, 4, -1]]), dtype=np.float32)
    dev = plan.device
    # one upload: [R, 4] near boxes (16-byte rows first), [R, n_dim] boxes, [R] class indexes
    host = np.concatenate([bv.reshape(-1).view(np.int32), boxes.reshape(-1).view(np.int32), cls])
    buf = torch.from_numpy(host).to(dev, non_blocking=True)
    d_bv, d_boxes, d_cls = buf[:4 * R], buf[4 * R:(4 + nd) * R], buf[(4 + nd) * R:]
    tab, out_rows, bases = plan.table(B)
    labels = torch.empty((out_rows,), dtype=torch.int32, device=dev)
    weights = torch.empty((out_rows,), dtype=torch.float32, device=dev)
    targets = torch.empty((out_rows, plan.code_size), dtype=torch.float32, device=dev)
    index = torch.empty((out_rows,), dtype=torch.int32, device=dev) if with_index else None
    overlap = torch.empty((max(R, 1),), dtype=torch.float32, device=dev)
    args = [_ptr(plan.anchors), _ptr(plan.anchors_bv), plan.anchors.shape[0], nd, tab, len(plan.rows),
            _ptr(d_boxes) if R else None, _ptr(d_bv) if R else None, _ptr(d_cls) if R else None, R,
            gt_off.ctypes.data_as(ctypes.c_void_p), B, int(plan.vec_encode), int(plan.linear_dim), int(plan.norm_velo),
            _ptr(labels), _ptr(targets), _ptr(weights), _ptr(index) if with_index else None, out_rows, _ptr(overlap)]
    if launch is None:
        lib.call("al3d_assign_targets_f32", *args, _stream())
    else:
        lib.call("al3d_assign_targets_launch_f32", *args, *(int(v) for v in launch), _stream())
    out = dict(labels=[], reg_targets=[], reg_weights=[], gt_index=[], gt_overlap=overlap[:R], gt_off=gt_off)
    for t, n in enumerate(plan.task_anchors):
        s = slice(bases[t], bases[t] + B * n)
        out["labels"].append(labels[s].view(B, n))
        out["reg_weights"].append(weights[s].view(B, n))
        out["reg_targets"].append(targets[s].view(B, n, plan.code_size))
        if with_index:
            out["gt_index"].append(index[s].view(B, n))
    return out
