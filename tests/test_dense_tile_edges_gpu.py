"""GPU suite: the pixel-tile pieces the dense conv kernels share (csrc/conv2d_tile.h) at the smallest shapes where they
can go wrong.  Every entry point is called directly (``lib.call``), so no environment knob picks the kernel; every case is
one launch on a map of a few hundred pixels.

Part 1: every entry point against the float64 convolution (tests/dense_fp64.py) on maps that are ragged in both directions
for all four pixel tiles (8 x 16, 4 x 32, 16 x 16, 4 x 8) and hold more than one tile per image, into a channel window of a
wider, sentinel-filled map.  Bounds are test_dense_gpu.py's: the f32-input kernel e < 1.5e-6 of the abs chain
(test_conv2d_bf16x6_is_fp32_faithful), bf16x6 e < 1.5e-6 and e < 2 e_f32 + 1e-8 (same test), every f16x3 kernel
dense_fp64.check_split_gate (test_conv2d_f16x3_is_fp32_class, test_conv3x3_winograd_f16x3_is_fp32_class).

Part 2: what needs no tolerance -- the batch index of the tile decode, the deconvolution's output phase, the fused GAP."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W = 2, 9, 35              # conv maps: 2 x 3 tiles of 8 x 16, 3 x 2 of 4 x 32, 1 x 3 of 16 x 16, 3 x 5 of 4 x 8, all ragged
DH, DW = 5, 19                  # deconv input maps: 1 x 2 ragged tiles of 8 x 16
COFF, PAD_C = 8, 24             # channel window: out[..., 8 : 8 + Cout] of an ldc = Cout + 24 map
FILL = -7.0

S2, P1, C3 = (3, 2, 1), (1, 1, 0), (3, 1, 1)        # (ksize, stride, pad); None = the 2x2 / stride-2 deconvolution


class Entry:
    """An entry point: its weight structure (detector_ops.dense_pack), arithmetic, call shape and channel counts."""
    def __init__(self, name, kind, math, form, cin=32, cout=40, gap=False, io=False):
        self.name, self.kind, self.math, self.form, self.cin, self.cout, self.gap, self.io = name, kind, math, form, cin, cout, gap, io
        self.needs_gap = gap and not io            # the ..._gap entry points; the LDS-DMA ones take a null buffer


E = {e.name: e for e in [
    Entry("al3d_conv2d_nhwc_f32", "f32", "f32", "conv"), Entry("al3d_deconv2x2_nhwc_f32", "f32", "f32", "deconv"),
    Entry("al3d_conv2d_nhwc_bf16x6", "bf16x6", "bf16x6", "conv"), Entry("al3d_deconv2x2_nhwc_bf16x6", "bf16x6", "bf16x6", "deconv"),
    Entry("al3d_conv2d_nhwc_f16x3", "f16x3", "f16x3", "conv"), Entry("al3d_deconv2x2_nhwc_f16x3", "f16x3", "f16x3", "deconv"),
    Entry("al3d_conv2d_nhwc_f16x3_gap", "f16x3", "f16x3", "conv", gap=True),
    Entry("al3d_deconv2x2_nhwc_f16x3_gap", "f16x3", "f16x3", "deconv", gap=True),
    Entry("al3d_conv2d_nhwc_f16x3_bstream", "bstream", "f16x3", "conv"),
    Entry("al3d_deconv2x2_nhwc_f16x3_bstream", "bstream", "f16x3", "deconv"),
    Entry("al3d_conv2d_nhwc_f16x3_dma", "dma", "f16x3", "conv", gap=True, io=True),
    Entry("al3d_deconv2x2_nhwc_f16x3_dma", "dma", "f16x3", "deconv", gap=True, io=True),
    Entry("al3d_conv3x3_nhwc_f16x3_frag", "frag3x3", "f16x3", "c3", cout=128),
    Entry("al3d_conv3x3_nhwc_f16x3_frag16", "frag16", "f16x3", "c3", cin=64, cout=128),
    Entry("al3d_conv3x3_nhwc_f16x3_wino", "wino", "f16x3", "c3", cout=128, io=True),
    Entry("al3d_conv3x3_res_nhwc_f16x3", "dma", "f16x3", "res", cout=128),
]}

# (entry point, geometry): the generic kernels at stride 2 / pad 1 and 1x1 / pad 0; 3x3 / s1 / p1 is the halo kernel of the
# bf16x6 and f16x3 entry points (Cin % 32 == 0) and the generic one of the others
MATRIX = [(n, g) for n in ("al3d_conv2d_nhwc_f32", "al3d_conv2d_nhwc_bf16x6", "al3d_conv2d_nhwc_f16x3", "al3d_conv2d_nhwc_f16x3_bstream",
                           "al3d_conv2d_nhwc_f16x3_dma", "al3d_conv2d_nhwc_f16x3_gap") for g in (S2, P1)]
MATRIX += [(n, C3) for n in ("al3d_conv2d_nhwc_bf16x6", "al3d_conv2d_nhwc_f16x3", "al3d_conv3x3_nhwc_f16x3_frag",
                             "al3d_conv3x3_nhwc_f16x3_frag16", "al3d_conv3x3_nhwc_f16x3_wino", "al3d_conv3x3_res_nhwc_f16x3")]
MATRIX += [(n, None) for n in E if E[n].form == "deconv"]


@functools.lru_cache(maxsize=None)
def _layer(geom, cin, cout, epi):
    """The layer (cin -> cout at geom) on the ragged map, shared by every entry point that runs it: inputs, the float64
    reference and abs chain, the f32-input kernel's output and its error.  epi "affine": scale, a shift that drives part of
    the outputs negative, ReLU; "null": no scale, no shift, no ReLU."""
    import dense_fp64 as R
    g = torch.Generator().manual_seed(1000 * cin + cout + (0 if geom is None else 7 * geom[0] + geom[1]))
    dec = geom is None
    x = torch.randn(B, cin, DH if dec else H, DW if dec else W, generator=g)
    taps = 4 if dec else geom[0] * geom[0]
    w = (torch.randn(cin, cout, 2, 2, generator=g) if dec else torch.randn(cout, cin, geom[0], geom[0], generator=g)) / (cin * taps) ** 0.5
    scale = shift = None
    if epi == "affine":
        scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.5
    relu = epi == "affine"
    ref, norm = R.deconv_fp64(x, w, scale, shift, relu) if dec else R.conv_fp64(x, w, geom[1], geom[2], scale, shift, relu)
    from al3d import detector_ops as D
    L = dict(geom=geom, cin=cin, cout=cout, epi=epi, relu=relu, xc=x, wc=w, scale_c=scale, shift_c=shift, x=R.nhwc(x).to(DEV),
             ref=ref, norm=norm, wp=(D.pack_deconv_weight(w) if dec else D.pack_conv_weight(w)).to(DEV),
             scale=None if scale is None else scale.to(DEV), shift=None if shift is None else shift.to(DEV))
    out, _ = _run(E["al3d_deconv2x2_nhwc_f32" if dec else "al3d_conv2d_nhwc_f32"], L, weights=(L["wp"], L["scale"]))
    assert torch.all(out[..., :COFF] == FILL) and torch.all(out[..., COFF + cout:] == FILL)
    L["e32"] = R.err(out[..., COFF:COFF + cout], ref, norm)
    return L


@functools.lru_cache(maxsize=None)
def _weights(kind, geom, cin, cout, epi):
    """(weights, scale) of the cached layer in structure `kind`'s format."""
    L = _layer(geom, cin, cout, epi)
    return _pack(kind, L["wp"], L["scale"])


def _pack(kind, wp, scale):
    from al3d import detector_ops as D
    w, sc = D.dense_pack(kind, wp, scale)
    return (w.data if isinstance(w, D.F16x3Packed) else w), sc


def _run(e, L, x=None, res=None, ldc=None, gap=False, weights=None):
    """One launch of entry point e on layer L (input x, L's own by default) into a sentinel-filled [.., ldc] map at COFF
    -> (map, gap partials or None)."""
    from al3d import detector_ops as D, lib
    from al3d.selector_ops import _ptr, _stream
    x = L["x"] if x is None else x
    w, sc = weights if weights is not None else _weights(e.kind, L["geom"], L["cin"], L["cout"], L["epi"])
    Bn, h, wd = x.shape[:3]
    dec = L["geom"] is None
    OH, OW = (2 * h, 2 * wd) if dec else ((h + 2 * L["geom"][2] - L["geom"][0]) // L["geom"][1] + 1,
                                         (wd + 2 * L["geom"][2] - L["geom"][0]) // L["geom"][1] + 1)
    ldc = L["cout"] + PAD_C if ldc is None else ldc
    out = torch.full((Bn, OH, OW, ldc), FILL, device=DEV)
    parts = None
    if gap:
        parts = torch.zeros((Bn, D.gap_parts(OH, OW, dec), ldc), device=DEV)
    args = [_ptr(x), _ptr(w), _ptr(sc), _ptr(L["shift"])]
    if e.form == "res":
        args += [_ptr(res)]
    args += [_ptr(out), Bn, h, wd, L["cin"], L["cout"]]
    if e.form == "conv":
        args += list(L["geom"])
    if e.form == "res":
        args += [res.shape[3]]
    args += [ldc, COFF, 1 if L["relu"] else 0]
    if e.gap:
        assert gap or not e.needs_gap
        args += [_ptr(parts), 0 if parts is None else parts.shape[1]]
    if e.io:
        args += [0]
    lib.call(e.name, *args, _stream())
    return out, parts


def _check_gate(e, err, e32, what):
    import dense_fp64 as R
    print(what, "e", err, "e_f32", e32)
    if e.math == "f32":
        assert err < R.E_MAX, (what, err)
    elif e.math == "bf16x6":
        assert e32 < R.E_MAX and err < R.E_MAX and err < 2.0 * e32 + 1e-8, (what, err, e32)
    else:
        R.check_split_gate(err, e32, what)


def _geom_id(g):
    return "deconv" if g is None else "k%ds%dp%d" % g


@pytest.mark.parametrize("epi", ["affine", "null"])
@pytest.mark.parametrize("name,geom", MATRIX, ids=[n[5:] + "-" + _geom_id(g) for n, g in MATRIX])
def test_entry_point_matches_float64_inside_its_window(name, geom, epi):
    import dense_fp64 as R
    e = E[name]
    L = _layer(geom, e.cin, e.cout, epi)
    if e.form == "res":
        # relu((conv * scale + shift) + res): the residual joins the reference and, by magnitude, the abs chain; the f32
        # yardstick is the f32-input kernel's stored window plus the same residual, each step rounded to f32
        g = torch.Generator().manual_seed(3)
        res = torch.randn(B, H, W, e.cout + 4, generator=g)
        rw = res[..., :e.cout]
        ref, norm = R.conv_fp64(L["xc"], L["wc"], 1, 1, L["scale_c"], L["shift_c"], False)
        ref, norm = ref + rw.double(), norm + rw.double().abs()
        y32 = _run(E["al3d_conv2d_nhwc_f32"], dict(L, relu=False), weights=(L["wp"], L["scale"]))[0][..., COFF:COFF + e.cout].cpu() + rw
        if L["relu"]:
            ref, y32 = torch.where(ref <= 0, torch.zeros_like(ref), ref), torch.where(y32 <= 0, torch.zeros_like(y32), y32)
        e32 = R.err(y32, ref, norm)
        out, _ = _run(e, L, res=res.to(DEV))
    else:
        ref, norm, e32 = L["ref"], L["norm"], L["e32"]
        out, _ = _run(e, L, gap=e.needs_gap)
    win = out[..., COFF:COFF + e.cout]
    assert tuple(win.shape) == tuple(ref.shape)
    _check_gate(e, R.err(win, ref, norm), e32, f"{name} {_geom_id(geom)} {epi}")
    assert torch.all(out[..., :COFF] == FILL) and torch.all(out[..., COFF + e.cout:] == FILL)       # the window, nothing else
    if epi == "affine":
        assert bool((win == 0).any()) and bool((win > 0).any())                                    # ReLU clipped some outputs, not all


@pytest.mark.parametrize("name,geom", [("al3d_conv3x3_nhwc_f16x3_frag", C3), ("al3d_conv2d_nhwc_f16x3_dma", S2),
                                       ("al3d_deconv2x2_nhwc_f16x3_dma", None)], ids=["frag", "dma", "dma-deconv"])
def test_untransposed_epilogue_of_the_16_byte_kernels(name, geom):
    """ldc = Cout + 25 is odd: the streamed 3x3 kernel and the LDS-DMA kernels store dwords straight from the fragment
    layout, through the shared epilogues.  Same gate, same window rule."""
    import dense_fp64 as R
    e = E[name]
    L = _layer(geom, e.cin, e.cout, "affine")
    out, _ = _run(e, L, ldc=e.cout + 25)
    _check_gate(e, R.err(out[..., COFF:COFF + e.cout], L["ref"], L["norm"]), L["e32"], name + " odd ldc")
    assert torch.all(out[..., :COFF] == FILL) and torch.all(out[..., COFF + e.cout:] == FILL)


# ---------------------------------------------------------------- part 2: no tolerance
BATCH_CASES = [(n, S2 if E[n].form == "conv" else None if E[n].form == "deconv" else C3) for n in E]


@pytest.mark.parametrize("name,geom", BATCH_CASES, ids=[n[5:] for n, _ in BATCH_CASES])
def test_zero_image_of_a_batch_gives_zero_output_in_both_batch_orders(name, geom):
    """Tile decode: with shift = 0 an all-zero image's output is exactly zero wherever it sits in the batch, and the other
    image's output does not depend on its place."""
    e = E[name]
    L = dict(_layer(geom, e.cin, e.cout, "affine"), shift=None)
    img = L["x"][:1]
    zero = torch.zeros_like(img)
    res0 = None
    outs = []
    for order in ((img, zero), (zero, img)):
        x = torch.cat(order).contiguous()
        if e.form == "res":
            res0 = torch.cat([torch.ones(1, H, W, e.cout, device=DEV) if o is img else torch.zeros(1, H, W, e.cout, device=DEV)
                              for o in order])
        out, _ = _run(e, L, x=x, res=res0, gap=e.needs_gap)
        outs.append(out[..., COFF:COFF + e.cout])
    assert torch.all(outs[0][1] == 0) and torch.all(outs[1][0] == 0)
    assert torch.equal(outs[0][0], outs[1][1]) and bool((outs[0][0] != 0).any())


@pytest.mark.parametrize("name", [n for n in E if E[n].form == "deconv" and not E[n].needs_gap])
def test_deconv_output_phase(name):
    """A one-hot input (pixel, channel) and weights whose value names (tap, cout): output pixel (2y + dy, 2x + dx) holds
    tap 2 dy + dx, exactly (small integers: exact in every arithmetic), every other pixel zero."""
    from al3d import detector_ops as D
    e = E[name]
    cin, cout, y, x, c = 32, 40, 3, 17, 5                  # (3, 17): second tile in x, not on a tile corner
    wt = torch.zeros(cin, cout, 2, 2)
    for dy in range(2):
        for dx in range(2):
            wt[c, :, dy, dx] = 1.0 + (2 * dy + dx) * 64 + torch.arange(cout)
    xin = torch.zeros(1, DH, DW, cin)
    xin[0, y, x, c] = 1.0
    L = dict(geom=None, cin=cin, cout=cout, relu=False, x=xin.to(DEV), scale=None, shift=None)
    out, _ = _run(e, L, weights=_pack(e.kind, D.pack_deconv_weight(wt).to(DEV), None))
    want = torch.zeros(1, 2 * DH, 2 * DW, cout)
    for dy in range(2):
        for dx in range(2):
            want[0, 2 * y + dy, 2 * x + dx] = wt[c, :, dy, dx]
    assert torch.equal(out[..., COFF:COFF + cout].cpu(), want)


@pytest.mark.parametrize("name,geom", [("al3d_conv2d_nhwc_f16x3_gap", S2), ("al3d_deconv2x2_nhwc_f16x3_gap", None),
                                       ("al3d_conv2d_nhwc_f16x3_dma", S2), ("al3d_deconv2x2_nhwc_f16x3_dma", None)],
                         ids=["f16x3", "f16x3-deconv", "dma", "dma-deconv"])
def test_fused_gap_is_the_mean_of_the_stored_output_and_repeats(name, geom):
    """The reduced partials against the float64 mean of the kernel's own stored f32 output (bound of
    test_gap_matches_two_stage_mean: rtol 1e-5, atol 1e-6), ragged tiles included; two runs give the same bits."""
    from al3d import detector_ops as D
    e = E[name]
    L = _layer(geom, e.cin, e.cout, "affine")
    out, parts = _run(e, L, gap=True)
    out2, parts2 = _run(e, L, gap=True)
    assert torch.equal(out, out2) and torch.equal(parts, parts2)
    win = out[..., COFF:COFF + e.cout]
    mean = D.gap_reduce_parts(parts, win.shape[1] * win.shape[2])[:, COFF:COFF + e.cout]
    assert torch.equal(mean, D.gap_reduce_parts(parts2, win.shape[1] * win.shape[2])[:, COFF:COFF + e.cout])
    want = win.double().mean(dim=(1, 2))
    torch.testing.assert_close(mean.cpu().double(), want.cpu(), rtol=1e-5, atol=1e-6)
    assert torch.all(parts[..., :COFF] == 0) and torch.all(parts[..., COFF + e.cout:] == 0)         # partials keep to the window
