"""Worker of tests/test_kernel_variants_gpu.py: ``python kernel_variant_worker.py CASE OUTDIR`` in a fresh process.

The C dispatchers read AL3D_FRAG_SHAPE, AL3D_FRAG_EPI, AL3D_F3_MAP, AL3D_DMA_STAGES, AL3D_DMA_PIPE, AL3D_DMA_EPI,
AL3D_R16_SHAPE, AL3D_R16_TPW, AL3D_SW2_NW128 and AL3D_TOK_MLP once per process, so a kernel variant is a property of the
process: the parent sets the environment, this script builds the case's inputs from a fixed seed, runs every layer of the
case through the public Python entry, checks each output against the float64 reference at the suite's own gates
(dense_fp64.py, spconv_fp64.py and test_spconv_fp64_gpu.Case) and writes the raw outputs to OUTDIR/<layer>.npy for the
parent to compare across environments.

Exit status: 0 = every gate held; 1 = a gate failed (traceback on stderr); 3 = the library refused the setting with an
Al3dError before anything was written."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import dense_fp64 as R2  # noqa: E402

DEV = "cuda:0"
OUT = {}


def save(key, t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert key not in OUT, key
    OUT[key] = np.ascontiguousarray(a, dtype=np.float32)


def _dense_inputs(g, B, H, W, Cin, Cout, k, deconv=False):
    x = torch.randn(B, Cin, H, W, generator=g) * torch.exp(torch.randn(B, Cin, H, W, generator=g))
    x = x.clamp(-6.0e4, 6.0e4)
    w = torch.randn(Cin, Cout, 2, 2, generator=g) / 8.0 if deconv else \
        torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(Cout, generator=g) * 0.1
    return x, w, scale, shift


# ------------------------------------------------------------------ the streamed 3x3 kernel (conv3x3_f16x3_frag_kernel)
FRAG_GEOMS = [(1, 128, 128, 256, 128), (3, 9, 70, 128, 256)]       # full BEV size (128 pixel tiles); ragged tiles


def case_frag():
    from al3d import detector_ops as D
    for B, H, W, Cin, Cout in FRAG_GEOMS:
        tag = f"frag_{B}x{H}x{W}x{Cin}x{Cout}"
        g = torch.Generator().manual_seed(Cin + H)
        x, w, scale, shift = _dense_inputs(g, B, H, W, Cin, Cout, 3)
        ref, norm = R2.conv_fp64(x, w, 1, 1, scale, shift, True)
        xd, wp = R2.nhwc(x).to(DEV), D.pack_conv_weight(w).to(DEV)
        e32 = R2.err(D.conv2d_nhwc(xd, wp, scale.to(DEV), shift.to(DEV), 3, 1, 1, True), ref, norm)
        w3, sc3 = D.split_f16x3(wp, scale.to(DEV))
        wf = D.pack_frag_f16x3(w3)
        plain = D.conv2d_nhwc(xd, wf, sc3, shift.to(DEV), 3, 1, 1, True)                    # f32 out
        e = R2.err(plain, ref, norm)
        print(f"{tag}: e = {e:.3e}, e_f32 = {e32:.3e}")
        R2.check_split_gate(e, e32, tag)
        wide = torch.full((B, H, W, Cout + 32), -3.0, device=DEV)                           # concat window
        D.conv2d_nhwc(xd, wf, sc3, shift.to(DEV), 3, 1, 1, True, out=wide, coff=32)
        assert torch.all(wide[..., :32] == -3.0), tag
        R2.check_split_gate(R2.err(wide[..., 32:], ref, norm), e32, tag + " window")
        pair = torch.full((B, H, W, Cout + 32), -3.0, device=DEV)                           # pair pixels out
        D.conv2d_nhwc(xd, wf, sc3, shift.to(DEV), 3, 1, 1, True, out=pair, coff=32, io=D.IO_OUT_PAIR)
        assert torch.all(pair[..., :32] == -3.0), tag
        want = D.rows_convert(wide[..., 32:].reshape(-1, Cout).contiguous(), True)
        assert torch.equal(pair[..., 32:].reshape(-1, Cout).view(torch.int32), want.view(torch.int32)), tag + " pair"
        odd = torch.full((B, H, W, Cout + 35), -3.0, device=DEV)        # coff % 4 == 1, ldc odd: the dword-store epilogue
        D.conv2d_nhwc(xd, wf, sc3, shift.to(DEV), 3, 1, 1, True, out=odd, coff=33)
        assert torch.equal(odd[..., 33:33 + Cout], wide[..., 32:]), tag + " unaligned window"
        assert torch.all(odd[..., :33] == -3.0) and torch.all(odd[..., 33 + Cout:] == -3.0), tag
        save(tag + "_f32", plain)
        save(tag + "_window", wide)
        save(tag + "_pair", pair)
        save(tag + "_unaligned", odd)


# ------------------------------------------------------------------ the LDS-DMA kernels (conv2d_f16x3_dma*_kernel)
DMA_GEOMS = [(2, 128, 128, 128, 256, 1, 1, 0), (1, 128, 128, 128, 256, 3, 2, 1), (2, 37, 21, 512, 236, 1, 1, 0),
             (1, 19, 50, 64, 40, 3, 1, 0), (1, 9, 11, 48, 16, 1, 1, 0), (3, 10, 9, 32, 300, 5, 2, 2),
             (2, 33, 20, 256, 200, "deconv", 2, 0)]


def case_dma():
    from al3d import detector_ops as D
    from al3d.lib import Al3dError
    for B, H, W, Cin, Cout, k, s, p in DMA_GEOMS:
        dec = k == "deconv"
        tag = f"dma_{B}x{H}x{W}x{Cin}x{Cout}_k{k}s{s}"
        g = torch.Generator().manual_seed(Cin + H + (2 if dec else k))
        x, w, scale, shift = _dense_inputs(g, B, H, W, Cin, Cout, k, dec)
        ref, norm = R2.deconv_fp64(x, w, scale, shift, True) if dec else R2.conv_fp64(x, w, s, p, scale, shift, True)
        OH, OW = ref.shape[1:3]
        xd = R2.nhwc(x).to(DEV)
        wp = (D.pack_deconv_weight(w) if dec else D.pack_conv_weight(w)).to(DEV)
        sd, td = scale.to(DEV), shift.to(DEV)

        def layer(xin, wgt, sc, **kw):
            return D.deconv2x2_nhwc(xin, wgt, sc, td, True, **kw) if dec else D.conv2d_nhwc(xin, wgt, sc, td, k, s, p, True, **kw)
        # the f32-input MFMA kernel takes Cin % 32 == 0; elsewhere (Cin = 48) there is no f32 structure to be within 3x of:
        # the absolute gate alone, and the bits of the LDS-staged f16x3 kernel below
        e32 = R2.err(layer(xd, wp, sd), ref, norm) if Cin % 32 == 0 else None
        w3, sc3 = D.split_f16x3(wp, sd)
        wd = D.pack_dma_f16x3(w3)
        staged = torch.full((B, OH, OW, Cout + 20), -3.0, device=DEV)
        layer(xd, w3, sc3, out=staged, coff=20)
        ldc = Cout + 20
        parts = D.gap_parts(OH, OW, dec)

        def run(xin, io, gap, coff=20):
            out = torch.full((B, OH, OW, Cout + coff), -3.0, device=DEV)
            layer(xin, wd, sc3, out=out, coff=coff, gap=gap, io=io)
            assert torch.all(out[..., :coff] == -3.0), tag
            return out
        base = run(xd, 0, None)                                                             # f32 in, f32 out, no GAP
        e = R2.err(base[..., 20:], ref, norm)
        print(f"{tag}: e = {e:.3e}, e_f32 = {e32}")
        if e32 is None:
            assert e < R2.E_MAX, f"{tag}: e = {e:.3e}"
        else:
            R2.check_split_gate(e, e32, tag)
        assert torch.equal(base, staged), tag + ": not the LDS-staged kernel's bits"
        gap = torch.full((B, parts + 3, ldc), -7.0, device=DEV)                             # with the fused GAP
        fused = run(xd, 0, gap)
        assert torch.equal(fused, base), tag + ": the fused GAP changed the map"
        assert torch.all(gap[:, parts:] == -7.0) and torch.all(gap[..., :20] == -7.0), tag
        mean = D.gap_reduce_parts(gap[:, :parts].contiguous(), OH * OW)[:, 20:].cpu().double()
        want = base[..., 20:].cpu().double().mean((1, 2))
        assert float((mean - want).abs().max()) <= 1e-5 * float(want.abs().max()), tag + ": fused GAP"
        save(tag + "_f32", base)
        save(tag + "_gap", gap)
        # pair pixels: the shipped kernel shape only (the library refuses them under AL3D_DMA_PIPE=0 / 4, 5 stages)
        xp = D.rows_convert(xd.view(-1, Cin), True).view_as(xd)
        try:
            pin = run(xp, D.IO_IN_PAIR, None)
        except Al3dError as exc:
            assert "pair pixels need the shipped kernel shape" in str(exc), exc
            continue
        assert torch.equal(pin, base), tag + ": pair pixels in"
        save(tag + "_pairin", pin)
        if Cout % 8 == 0:
            b24 = run(xd, 0, None, coff=24)
            pout = run(xd, D.IO_OUT_PAIR, None, coff=24)
            want = D.rows_convert(b24[..., 24:].reshape(-1, Cout).contiguous(), True)
            assert torch.equal(pout[..., 24:].reshape(-1, Cout).view(torch.int32), want.view(torch.int32)), tag + " pair out"
            save(tag + "_pairout", pout)


# ------------------------------------------------------------------ sparse layers
def _sparse_case(seed, cin, cout, geom, xmag, residual, raster):
    from test_detector_oracle import random_sparse
    from test_spconv_fp64_gpu import Case, _raster
    rng = np.random.default_rng(seed)
    shape, batch, n = [9, 41, 37], 3, 3001                 # 3001 rows = 93 tiles of 32 + a ragged tile of 25
    _, coords = random_sparse(rng, batch, shape, n, 1)
    if raster:
        coords = coords[_raster(coords, shape)]
    case = Case(rng, coords, batch, shape, cin, cout, geom, xmag)
    if not residual and case.res is not None:
        case.res = None
        case.reference()
    return case


def case_r16():
    """The item-stream kernel of level 0 (sp_conv_r16_kernel).  AL3D_R16_TPW reaches the C dispatcher only while
    detector_ops passes tiles_per_wave = 0, so R16_TPW (read from the same variable) is zeroed for the saved runs; the
    argument route is run beside it."""
    from al3d import detector_ops as D
    from test_spconv_fp64_gpu import check_structures
    env_tpw = D.R16_TPW
    for cin, cout, geom, residual, xmag in [(16, 16, "subm", True, 1.0), (16, 16, "subm", False, 1e-4), (16, 32, "down", False, 1.0)]:
        tag = f"r16_{geom}_{cin}x{cout}_res{int(residual)}"
        case = _sparse_case(cin * 100 + cout + residual, cin, cout, geom, xmag, residual, True)
        D.R16_TPW = 0
        errs = check_structures(case, [True, "r16_f16x3"], tag)        # the float64 gates (restores R16_TPW = 0)
        print(tag, {str(m): f"{e:.3e}" for m, e in errs.items()})
        got = case.run("r16_f16x3")
        save(tag, got)
        for tpw in (4, 8, 16, 32):                                     # tiles_per_wave as an argument
            D.R16_TPW = tpw
            assert np.array_equal(case.run("r16_f16x3"), got), f"{tag}: tiles_per_wave = {tpw} changed the output"
        D.R16_TPW = env_tpw


def case_sw2():
    """The register-gather wave kernel at 128 output channels (sp_conv_wave2_kernel<*, 128, 8 | 16, ..>), every row format."""
    from al3d import detector_ops as D
    from test_spconv_fp64_gpu import check_structures
    for cin, cout, geom in [(64, 128, "down"), (128, 128, "subm")]:
        tag = f"sw2_{geom}_{cin}x{cout}"
        case = _sparse_case(cin + cout, cin, cout, geom, 1.0, True, False)
        errs = check_structures(case, [True, "wave2_f16x3", "wave2_f16x3_tiles"], tag)
        print(tag, {str(m): f"{e:.3e}" for m, e in errs.items()})
        save(tag + "_plain", case.run("wave2_f16x3"))
        save(tag + "_tiles", case.run("wave2_f16x3_tiles"))
        ios = [D.IO_IN_PAIR, D.IO_OUT_PAIR, D.IO_IN_PAIR | D.IO_OUT_PAIR]
        if case.res is not None:
            ios += [D.IO_RES_PAIR, D.IO_IN_PAIR | D.IO_OUT_PAIR | D.IO_RES_PAIR]
        for io in ios:                                     # the gate of test_spconv_fp64_gpu.test_pair_rows_vs_fp64
            floor = (case.floor if io & D.IO_IN_PAIR else 0.0) + 2.0 ** -36 * (bool(io & D.IO_OUT_PAIR) + bool(io & D.IO_RES_PAIR))
            got = case.run("wave2_f16x3_tiles", io=io)
            e = case.err_floor(got, floor)
            assert e <= 1.5e-6, f"{tag} io={io}: e = {e:.3e}"
            save(f"{tag}_io{io}", got)


# ------------------------------------------------------------------ the fused token MLP (tok_mlp_f16x3_kernel)
TOK_SHAPES = [(1000, 96), (129, 96), (257, 96), (32, 96), (1000, 192), (193, 192), (385, 192), (16, 192), (5, 192)]


def case_tok():
    from al3d import token_ops as Tk
    for T_, C in TOK_SHAPES:
        g = torch.Generator().manual_seed(T_ + C)
        x = (torch.randn(T_, C, generator=g) * 1.7 + 0.3)
        ln_w, ln_b = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
        w1, b1 = torch.randn(4 * C, C, generator=g) / C ** 0.5, torch.randn(4 * C, generator=g) * 0.1
        w2, b2 = torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5, torch.randn(C, generator=g) * 0.1
        ref = R2.mlp_fp64(x, ln_w, ln_b, w1, b1, w2, b2, 1e-5)
        dev = lambda t: t.to(DEV)                                                            # noqa: E731
        pk = Tk.PackedMlp(dev(ln_w), dev(ln_b), 1e-5, dev(w1), dev(b1), dev(w2), dev(b2))
        got = Tk.mlp(dev(x).clone(), pk)
        f1, f2 = Tk.PackedLinear(dev(w1), dev(b1)), Tk.PackedLinear(dev(w2), dev(b2))
        xs = dev(x).clone()
        hid = Tk.linear(Tk.layernorm(xs, dev(ln_w), dev(ln_b), 1e-5, pair=True), f1, a_pair=True, act="gelu", out_pair=True)
        split = Tk.linear(hid, f2, a_pair=True, residual=xs, out=xs).cpu().double()
        scale = float(ref.abs().max())
        e_fused, e_split = float((got.cpu().double() - ref).abs().max()), float((split - ref).abs().max())
        print(f"tok_{T_}x{C}: fused {e_fused / scale:.3e} split {e_split / scale:.3e}")
        assert e_fused <= 3.0 * e_split + 1e-7 * scale, (T_, C, e_fused, e_split, scale)
        assert e_fused <= 1e-5 * scale, (T_, C, e_fused, scale)
        save(f"tok_{T_}x{C}", got)


CASES = {"frag": case_frag, "dma": case_dma, "r16": case_r16, "sw2": case_sw2, "tok": case_tok}


def main():
    name, outdir = sys.argv[1], sys.argv[2]
    from al3d.lib import Al3dError
    try:
        with torch.no_grad():
            CASES[name]()
        torch.cuda.synchronize()
    except Al3dError as exc:
        print(f"Al3dError: {exc}", file=sys.stderr)
        return 3
    os.makedirs(outdir, exist_ok=True)
    for key, a in OUT.items():
        np.save(os.path.join(outdir, key + ".npy"), a)
    print(f"{name}: {len(OUT)} outputs written")
    return 0


if __name__ == "__main__":
    sys.exit(main())
