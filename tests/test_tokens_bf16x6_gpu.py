"""GPU suite: the token kernels in bf16x6 arithmetic (csrc/tokens_bf16x6.hip; ``AL3D_MATH=bf16x6`` / ``f32`` on the token
path) against float64 on the host side of the comparison, at the bounds the f16x3 kernels are held to (tests/test_swin_gpu.py,
tests/test_transfusion_gpu.py) -- and at magnitudes the f16x3 kernels cannot take: operands beyond 65504 and far below
f16's normal range.

Bounds.  GEMM: error <= 1.5e-6 of sum|a||w| + |b| and <= 3x torch's fp32 GEMM error + 1e-7 (test_token_gemm_is_fp32_class).
Epilogues: the GEMM's bound carried through the epilogue -- ReLU is 1-Lipschitz; a folded scale multiplies value and
normaliser alike; a residual adds one fp32 rounding of the sum, so |residual| joins the normaliser; GELU <= 3e-6 absolute
at O(1) pre-activations (test_token_gemm_epilogues).  Attention: e <= 3 e32 + 2e-6 (1e-6 for mha16) and e <= 1e-5, absolute
at O(1) values as in test_window_attention_kernel_matches_float64 / test_mha16_kernel_matches_float64; where v is scaled by
3e5 the output scales with it exactly, so both sides are divided by that factor."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def bf16x6(monkeypatch):
    from al3d import detector_ops as D
    monkeypatch.setattr(D, "MATH", "bf16x6")


# ------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("xmag", [1.0, 1e-4, 300.0, 3e5])
@pytest.mark.parametrize("M,K,N", [(5, 192, 576), (257, 96, 96), (130, 48, 100), (64, 3072, 768)])
def test_token_gemm_is_fp32_class_over_the_fp32_range(M, K, N, xmag):
    from al3d import token_ops as T
    g = torch.Generator().manual_seed(M + K)
    a = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, K, generator=g)) * xmag).to(DEV)      # no clamp
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b = (torch.randn(N, generator=g) * 0.1).to(DEV)
    pk = T.PackedLinear(w, b)
    ref = a.double() @ w.double().t() + b.double()
    scale = a.abs().double() @ w.abs().double().t() + b.abs().double()
    got = T.linear(a, pk)
    e6 = float(((got.double() - ref).abs() / scale).max())
    e32 = float((((a @ w.t() + b).double() - ref).abs() / scale).max())
    print(f"M={M} K={K} N={N} xmag={xmag}: e6={e6:.3e} e32={e32:.3e} max|a|={float(a.abs().max()):.3e}")
    if xmag == 3e5:
        assert float(a.abs().max()) > 65504.0 and bool(torch.isfinite(got).all())
    assert e6 < 1.5e-6 and e6 < 3.0 * e32 + 1e-7, (e6, e32)


@pytest.fixture(scope="module")
def epi():
    """One (130, 96, 96) problem for the epilogue tests: a partial row tile and a partial column block."""
    g = torch.Generator().manual_seed(11)
    M, K, N = 130, 96, 96
    a = torch.randn(M, K, generator=g).to(DEV)
    w, b = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV), torch.randn(N, generator=g).to(DEV)
    s = (torch.rand(N, generator=g) * 4.0 - 2.0).to(DEV)
    prod = a.double() @ w.double().t()
    aprod = a.abs().double() @ w.abs().double().t()
    return dict(M=M, K=K, N=N, a=a, w=w, b=b, s=s, prod=prod, aprod=aprod, g=g)


def test_gemm_gelu_and_relu(epi):
    from al3d import token_ops as T
    pk = T.PackedLinear(epi["w"], epi["b"])
    lin = epi["prod"] + epi["b"].double()
    norm = epi["aprod"] + epi["b"].abs().double()
    got = T.linear(epi["a"], pk, act="gelu")
    e = float((got.double() - F.gelu(lin)).abs().max())
    print(f"gelu: max abs error {e:.3e}")
    assert e <= 3e-6
    got = T.linear(epi["a"], pk, act="relu")
    e = float(((got.double() - lin.clamp(min=0.0)).abs() / norm).max())
    print(f"relu: {e:.3e} of sum|a||w|+|b|")
    assert e < 1.5e-6 and bool((got >= 0).all()) and bool((got == 0).any())


def test_gemm_folded_scale_without_bias(epi):
    from al3d import token_ops as T
    pk = T.PackedLinear(epi["w"], None, scale=epi["s"])
    got = T.linear(epi["a"], pk)
    ref = epi["prod"] * epi["s"].double()
    e = float(((got.double() - ref).abs() / (epi["aprod"] * epi["s"].abs().double())).max())
    print(f"scale, no bias: {e:.3e}")
    assert e < 1.5e-6


def test_gemm_residual_may_alias_out(epi):
    from al3d import token_ops as T
    pk = T.PackedLinear(epi["w"], epi["b"])
    res = torch.randn(epi["M"], epi["N"], generator=torch.Generator().manual_seed(5)).to(DEV)
    stream = res.clone()
    out = T.linear(epi["a"], pk, residual=stream, out=stream)
    assert out.data_ptr() == stream.data_ptr()
    ref = epi["prod"] + epi["b"].double() + res.double()
    norm = epi["aprod"] + epi["b"].abs().double() + res.abs().double()
    e = float(((out.double() - ref).abs() / norm).max())
    print(f"aliased residual: {e:.3e}")
    assert e < 1.5e-6


def test_gemm_rowmap_drops_and_permutes(epi):
    from al3d import token_ops as T
    M, N, R, rows_out = epi["M"], epi["N"], 101, 150
    pk = T.PackedLinear(epi["w"], epi["b"])
    g = torch.Generator().manual_seed(6)
    perm = torch.randperm(M, generator=g)
    dest = torch.randperm(rows_out, generator=g)[:R].to(torch.int32)
    rowmap = torch.full((M,), -1, dtype=torch.int32)
    rowmap[perm[:R]] = dest                                  # R of the M rows land on scattered rows, the rest are dropped
    rowmap = rowmap.to(DEV)
    out = T.linear(epi["a"], pk, rowmap=rowmap, out_rows=rows_out)
    assert tuple(out.shape) == (rows_out, N)
    lin = epi["prod"] + epi["b"].double()
    norm = epi["aprod"] + epi["b"].abs().double()
    live = rowmap >= 0
    e = float(((out[rowmap[live].long()].double() - lin[live]).abs() / norm[live]).max())
    untouched = torch.ones(rows_out, dtype=torch.bool, device=DEV)
    untouched[rowmap[live].long()] = False
    print(f"rowmap: {e:.3e}; {int(untouched.sum())} untouched rows")
    assert e < 1.5e-6 and int(untouched.sum()) == rows_out - R and bool((out[untouched] == 0).all())
    # scatter-add into a residual stream, in place
    res = torch.randn(rows_out, N, generator=g).to(DEV)
    stream = res.clone()
    out = T.linear(epi["a"], pk, residual=stream, rowmap=rowmap)
    assert out.data_ptr() == stream.data_ptr()
    ref = res.double().clone()
    ref[rowmap[live].long()] += lin[live]
    assert torch.equal(out[untouched], res[untouched])
    assert float(((out.double() - ref).abs()[rowmap[live].long()] / (norm[live] + res.abs().double()[rowmap[live].long()])).max()) < 1.5e-6


def test_gemm_refuses_bad_arguments(epi):
    from al3d import token_ops as T
    from al3d.lib import Al3dError
    pk = T.PackedLinear(epi["w"], epi["b"])
    with pytest.raises(Al3dError):
        T.linear(epi["a"][:, :40].contiguous(), pk)            # K mismatch
    with pytest.raises(Al3dError):
        T.linear(epi["a"], pk, a_pair=True)
    with pytest.raises(Al3dError):
        T.linear(epi["a"], pk, out=torch.empty(epi["M"], epi["N"] + 2, device=DEV))       # ldc no multiple of 4


def test_window_attention_refuses_2_31_items():
    """nwin * heads = 2^31 (window, head) items do not fit a grid: both window-order entries refuse them by name.  (Without
    the check the launch itself fails as an invalid configuration: no kernel ever runs over these small tensors.)"""
    from al3d import lib
    qkv, out = torch.zeros(49, 3 * 1024, device=DEV), torch.zeros(49, 1024, device=DEV)
    table = torch.zeros(169, 32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    nwin, C, heads = 2 ** 26, 1024, 32
    with pytest.raises(lib.Al3dError, match="too many"):
        lib.call("al3d_tok_window_attention_f32", qkv.data_ptr(), table.data_ptr(), nwin, C, heads, 1, 1, 0, 32 ** -0.5, 0,
                 out.data_ptr(), stream)
    with pytest.raises(lib.Al3dError, match="too many"):
        lib.call("al3d_tok_window_attention_bf16x6", qkv.data_ptr(), table.data_ptr(), nwin, C, heads, 1, 1, 0, 32 ** -0.5,
                 out.data_ptr(), stream)


def test_nonfinite_input_propagates():
    from al3d import token_ops as T
    g = torch.Generator().manual_seed(2)
    a = torch.randn(40, 32, generator=g).to(DEV)
    a[3, 5], a[7, 0] = float("inf"), float("nan")
    got = T.linear(a, T.PackedLinear(torch.randn(16, 32, generator=g).to(DEV)))
    bad = ~torch.isfinite(got).all(dim=1)
    assert bad.nonzero().flatten().tolist() == [3, 7]
    qkv = torch.randn(49, 3 * 32, generator=g).to(DEV)
    qkv[11, 70] = float("inf")                               # a v entry: every query of the window sees it
    out = T.window_attention(qkv, torch.zeros(169, 1, device=DEV), 1, 1, 1, 0, 32 ** -0.5)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(out[:, 6]).any()) and bool(torch.isfinite(out[:, :6]).all())


# ------------------------------------------------------------------ attention
REGIMES = {"unit": (1.0, 1.0, 1.0), "v3e5": (1.0, 1.0, 3e5), "q1e5_k1e-5": (1e5, 1e-5, 1.0)}


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("B,H,W,shift", [(1, 7, 7, 0), (2, 10, 13, 0), (2, 10, 13, 3)])
def test_window_attention_matches_float64_in_both_orders(B, H, W, shift, regime):
    """Window order against the restatement's WindowMSA core in float64; token order (shift, padding with the qkv bias row
    and window partition done by the kernel) must give the same bits through the row map."""
    import swin_torch as R
    from al3d import token_ops as T
    from al3d.models.swin import ShiftWindowMSA
    heads, C = 3, 96
    qs, ks, vs = REGIMES[regime]
    g = torch.Generator().manual_seed(H * W + shift)
    attn = ShiftWindowMSA(C, heads, 7, shift)
    attn.w_msa.relative_position_bias_table.data = torch.randn(169, heads, generator=g) * 0.7
    attn = attn.to(DEV).eval()
    m = attn.w_msa
    table = m.relative_position_bias_table.detach()
    mult = torch.cat([torch.full((C,), qs), torch.full((C,), ks), torch.full((C,), vs)])
    tok = ((torch.randn(B * H * W, 3 * C, generator=g) * 1.5) * mult).to(DEV)
    bias = ((torch.randn(3 * C, generator=g) * 1.5) * mult).to(DEV)
    rowmap, (nwy, nwx) = T.window_rowmap(B, H, W, 7, shift)
    rowmap = torch.from_numpy(rowmap).to(DEV).long()
    nwin = B * nwy * nwx
    qkv = torch.where((rowmap >= 0)[:, None], tok[rowmap.clamp(min=0)], bias[None, :]).contiguous()      # window order
    if regime != "unit":
        assert float(qkv.abs().max()) > 65504.0

    def core(dtype):
        x = qkv.to(dtype).view(nwin, 49, 3, heads, 32).permute(2, 0, 3, 1, 4)
        q, k, v = x[0], x[1], x[2]
        a = (q * m.scale) @ k.transpose(-2, -1)
        b = table.to(dtype)[m.relative_position_index.view(-1)].view(49, 49, -1)
        a = a + b.permute(2, 0, 1).unsqueeze(0)
        if shift:
            Hp, Wp = nwy * 7, nwx * 7
            img = torch.zeros((1, Hp, Wp, 1), device=DEV, dtype=dtype)
            cnt = 0
            for hs in (slice(0, -7), slice(-7, -shift), slice(-shift, None)):
                for ws_ in (slice(0, -7), slice(-7, -shift), slice(-shift, None)):
                    img[:, hs, ws_, :] = cnt
                    cnt += 1
            mw = R._window_partition(img, 7).view(-1, 49)
            am = mw.unsqueeze(1) - mw.unsqueeze(2)
            am = am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0)
            a = (a.view(B, nwy * nwx, heads, 49, 49) + am.unsqueeze(1).unsqueeze(0)).view(-1, heads, 49, 49)
        return (a.softmax(-1) @ v).transpose(1, 2).reshape(nwin * 49, C)

    with torch.no_grad():
        ref, ref32 = core(torch.float64), core(torch.float32)
    got = T.window_attention(qkv, table, heads, nwy, nwx, shift, m.scale)
    e = float((got.double() - ref).abs().max()) / vs
    e32 = float((ref32.double() - ref).abs().max()) / vs
    print(f"B={B} H={H} W={W} shift={shift} {regime}: e={e:.3e} e32={e32:.3e}")
    assert bool(torch.isfinite(got).all())
    assert e <= 3.0 * e32 + 2e-6 and e <= 1e-5, (e, e32)
    got_tok = T.window_attention_tokens(tok, bias, table, B, H, W, heads, shift, m.scale)
    live = rowmap >= 0
    assert sorted(rowmap[live].tolist()) == list(range(B * H * W))
    assert torch.equal(got_tok[rowmap[live]], got[live])


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("B,Pq,Pk", [(1, 5, 40), (2, 37, 1100)])
def test_mha16_matches_float64(B, Pq, Pk, regime):
    """A partial query tile with one key chunk, and two key chunks through the combine kernel; q / k / v as column slices
    of wider matrices."""
    from al3d import token_ops as T
    heads, C = 8, 128
    qs, ks, vs = REGIMES[regime]
    g = torch.Generator().manual_seed(Pq + Pk)
    qm = (torch.randn(B * Pq, 3 * C, generator=g) * 1.3 * qs).to(DEV)
    km = (torch.randn(B * Pk, 2 * C, generator=g) * 1.3).to(DEV)
    km[:, :C] *= ks
    km[:, C:] *= vs
    q, k, v = qm[:, C:2 * C], km[:, :C], km[:, C:]

    def core(dt):
        def hf(x, L):
            return x.to(dt).reshape(B, L, heads, 16).permute(0, 2, 1, 3)
        w = torch.softmax((hf(q, Pq) * 0.25) @ hf(k, Pk).transpose(-1, -2), dim=-1)
        return (w @ hf(v, Pk)).permute(0, 2, 1, 3).reshape(B * Pq, C)
    ref, ref32 = core(torch.float64), core(torch.float32)
    got = T.mha16(q, k, v, B, Pq, Pk, heads, 0.25)
    e, e32 = float((got.double() - ref).abs().max()) / vs, float((ref32.double() - ref).abs().max()) / vs
    print(f"B={B} Pq={Pq} Pk={Pk} {regime}: e={e:.3e} e32={e32:.3e}")
    assert bool(torch.isfinite(got).all())
    assert e <= 3.0 * e32 + 1e-6 and e <= 1e-5, (e, e32)


# ------------------------------------------------------------------ modules
def test_swin_t_matches_restatement_under_bf16x6():
    """The whole backbone at the smallest size of test_swin_t_matches_restatement, against the torch restatement in
    float64, with that test's bound per output level."""
    import swin_torch as R
    from al3d.models.swin import SwinTransformer
    from al3d.synthetic import seed_modules_
    swin = seed_modules_(SwinTransformer(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7,
                                         mlp_ratio=4, qkv_bias=True, patch_norm=True, out_indices=[1, 2, 3]), 23).to(DEV)
    B, H, W = 2, 96, 160
    img = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(9)).to(DEV)
    with torch.no_grad():
        got = swin(img)
        again = swin(img)
        ref32 = R.swin(swin, img)
        ref = R.swin(swin.double(), img, torch.float64)
        swin.float()
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    for lvl, (o, r32) in enumerate(zip(got, ref32)):
        assert o.shape == r32.shape and bool(torch.isfinite(o).all())
        s = float(r32.abs().max())
        e, e32 = float((o.double() - ref[lvl]).abs().max()), float((r32.double() - ref[lvl]).abs().max())
        print(f"level {lvl}: e={e:.3e} e32={e32:.3e} scale={s:.3e}")
        assert e <= 3.0 * e32 + 2e-6 * s, (lvl, e, e32, s)


def test_transfusion_decoder_layer_matches_the_reference_module_under_bf16x6():
    """tests/golden/bevfusion_decoder_layer.npz (the reference's TransformerDecoderLayer on the CPU) at the tolerance of
    test_transfusion_decoder_layer_matches_the_reference_module."""
    from al3d.models.transfusion_head import PositionEmbeddingLearned, TransformerDecoderLayer
    z = np.load(os.path.join(GOLD, "bevfusion_decoder_layer.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    t = lambda k: torch.from_numpy(z[k])                                   # noqa: E731
    C, heads, ffn = (int(v) for v in z["cfg"])
    layer = TransformerDecoderLayer(C, heads, ffn, dropout=0.1, activation="relu", self_posembed=PositionEmbeddingLearned(2, C),
                                    cross_posembed=PositionEmbeddingLearned(2, C))
    missing, unexpected = layer.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    layer = layer.to(DEV).eval()
    query, key, key_pos = t("query"), t("key"), t("key_pos")               # [B, C, Pq], [B, C, Pk]
    B, _, Pq = query.shape
    rows = lambda x: x.permute(0, 2, 1).reshape(-1, x.shape[1]).contiguous()      # noqa: E731
    with torch.no_grad():
        got = layer(rows(query).to(DEV), rows(key).to(DEV), t("query_pos").reshape(B * Pq, 2).to(DEV),
                    key_pos[0].contiguous().to(DEV), B).cpu()
    ref = rows(t("out"))
    assert got.shape == ref.shape == (B * Pq, C)
    e = float((got - ref).abs().max())
    print(f"decoder layer: max abs error {e:.3e} at scale {float(ref.abs().max()):.3e}")
    assert e <= 2e-4 * float(ref.abs().max()) + 1e-6, e
