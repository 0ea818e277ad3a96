"""CPU suite: which C-ABI entry the token ops issue under each ``detector_ops.MATH``, with ``lib.call`` recorded instead of
run.  f16x3 issues the entries of csrc/tokens.hip with the argument lists it always had; bf16x6 and f32 issue the
``_bf16x6`` entries of csrc/tokens_bf16x6.hip (no pair rows, no fused Swin kernel); a ``PackedLinear`` builds each
arithmetic's weight image once, however often the arithmetic flips."""
import pytest
import torch


@pytest.fixture
def rec(monkeypatch):
    """Record (name, args) of every lib.call; device checks and the stream lookup accept CPU tensors."""
    from al3d import detector_ops as D, lib, token_ops as T
    calls = []
    monkeypatch.setattr(lib, "call", lambda name, *args: calls.append((name, args)))

    def dev(t, dtype, name):
        if t is None:
            return None
        assert isinstance(t, torch.Tensor) and t.dtype == dtype, name
        return t.contiguous()
    for mod in (D, T):
        monkeypatch.setattr(mod, "_dev", dev)
        monkeypatch.setattr(mod, "_stream", lambda: 77)
    monkeypatch.setattr(D, "MATH", "f16x3")
    return calls


def _names(calls):
    return [c[0] for c in calls]


def _p(t):
    return None if t is None else t.data_ptr()


def _linear_case():
    from al3d import token_ops as T
    g = torch.Generator().manual_seed(1)
    a, res = torch.randn(10, 32, generator=g), torch.randn(12, 24, generator=g)
    rowmap = torch.arange(10, dtype=torch.int32)
    pk = T.PackedLinear(torch.randn(24, 32, generator=g), torch.randn(24, generator=g), scale=torch.rand(24, generator=g))
    return a, res, rowmap, pk


def test_f16x3_issues_todays_calls(rec, monkeypatch):
    from al3d import token_ops as T
    a, res, rowmap, pk = _linear_case()
    assert T.arithmetic() == "f16x3" and T.pair_rows() is True
    out = T.linear(a, pk, a_pair=True, act="gelu", residual=res, rowmap=rowmap, out_pair=True)
    image, scale = pk.packed("f16x3")
    assert image is pk.image and scale is pk.scale and image.dtype == torch.float16 and scale.shape == (24,)
    assert out is res
    assert rec[-1] == ("al3d_tok_linear_f16x3", (_p(a), 1, _p(image), _p(scale), _p(pk.bias), 10, 32, 24, 1, _p(res), 24,
                                                 _p(rowmap), _p(res), 24, 1, 77))
    out = T.linear(a, pk)
    assert rec[-1] == ("al3d_tok_linear_f16x3", (_p(a), 0, _p(image), _p(scale), _p(pk.bias), 10, 32, 24, 0, None, 0,
                                                 None, _p(out), 24, 0, 77))
    qkv, table, bias = torch.zeros(2 * 49, 3 * 96), torch.zeros(169, 3), torch.zeros(3 * 96)
    out = T.window_attention(qkv, table, 3, 1, 2, 3, 0.125)
    assert rec[-1] == ("al3d_tok_window_attention_f32", (_p(qkv), _p(table), 2, 96, 3, 1, 2, 3, 0.125, 1, _p(out), 77))
    out = T.window_attention(qkv, table, 3, 1, 2, 0, 0.125, pair=False)
    assert rec[-1] == ("al3d_tok_window_attention_f32", (_p(qkv), _p(table), 2, 96, 3, 1, 2, 0, 0.125, 0, _p(out), 77))
    tok = torch.zeros(2 * 5 * 6, 3 * 96)
    out = T.window_attention_tokens(tok, bias, table, 2, 5, 6, 3, 3, 0.125)
    assert rec[-1] == ("al3d_tok_window_attention_tokens_f32", (_p(tok), _p(bias), _p(table), 2, 5, 6, 96, 3, 3, 0.125, 1,
                                                                _p(out), 77))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    wide = torch.zeros(2 * 40, 3 * 128)
    q, k, v = wide[:10, :128], wide[:, 128:256], wide[:, 256:]
    out = T.mha16(q, k, v, 2, 5, 40, 8, 0.25)
    name, args = rec[-1]
    assert name == "al3d_tok_mha16_f32"
    assert args[:11] == (q.data_ptr(), 384, k.data_ptr(), 384, v.data_ptr(), 384, 2, 8, 5, 40, 0.25)
    assert args[11:13] == (_p(out), 128) and args[14] == 77 and len(args) == 15


@pytest.mark.parametrize("math", ["bf16x6", "f32"])
def test_other_arithmetics_issue_the_bf16x6_entries(rec, monkeypatch, math):
    from al3d import detector_ops as D, token_ops as T
    monkeypatch.setattr(D, "MATH", math)
    a, res, rowmap, pk = _linear_case()
    assert T.arithmetic() == "bf16x6" and T.pair_rows() is False
    out = T.linear(a, pk, act="relu", residual=res, rowmap=rowmap)
    planes, scale = pk.packed("bf16x6")
    assert planes.dtype == torch.bfloat16 and tuple(planes.shape) == (3, 24, 32) and scale is pk.scale_in
    assert rec[-1] == ("al3d_tok_linear_bf16x6", (_p(a), _p(planes), _p(scale), _p(pk.bias), 10, 32, 24, 2, _p(res), 24,
                                                  _p(rowmap), _p(res), 24, 77))
    assert out is res
    plain = T.PackedLinear(torch.zeros(8, 16))               # no folded scale, no bias: two null pointers
    out = T.linear(a[:, :16].contiguous(), plain)
    assert rec[-1][1][2:4] == (None, None) and rec[-1][0] == "al3d_tok_linear_bf16x6"
    qkv, table, bias = torch.zeros(2 * 49, 3 * 96), torch.zeros(169, 3), torch.zeros(3 * 96)
    out = T.window_attention(qkv, table, 3, 1, 2, 3, 0.125)
    assert rec[-1] == ("al3d_tok_window_attention_bf16x6", (_p(qkv), _p(table), 2, 96, 3, 1, 2, 3, 0.125, _p(out), 77))
    tok = torch.zeros(2 * 5 * 6, 3 * 96)
    out = T.window_attention_tokens(tok, bias, table, 2, 5, 6, 3, 3, 0.125)
    assert rec[-1] == ("al3d_tok_window_attention_tokens_bf16x6", (_p(tok), _p(bias), _p(table), 2, 5, 6, 96, 3, 3, 0.125,
                                                                   _p(out), 77))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    wide = torch.zeros(2 * 40, 3 * 128)
    T.mha16(wide[:10, :128], wide[:, 128:256], wide[:, 256:], 2, 5, 40, 8, 0.25)
    assert rec[-1][0] == "al3d_tok_mha16_bf16x6" and len(rec[-1][1]) == 15
    assert not [n for n in _names(rec) if n.endswith("_f16x3") or n in ("al3d_tok_window_attention_f32", "al3d_tok_mha16_f32")]


@pytest.mark.parametrize("math", ["bf16x6", "f32"])
def test_pair_rows_and_fused_kernels_are_refused(rec, monkeypatch, math):
    from al3d import detector_ops as D, token_ops as T
    from al3d.lib import Al3dError
    monkeypatch.setattr(D, "MATH", math)
    a, res, rowmap, pk = _linear_case()
    qkv, table, bias = torch.zeros(49, 3 * 96), torch.zeros(169, 3), torch.zeros(3 * 96)
    for bad in (lambda: T.linear(a, pk, a_pair=True), lambda: T.linear(a, pk, out_pair=True),
                lambda: T.window_attention(qkv, table, 3, 1, 1, 0, 0.125, pair=True),
                lambda: T.window_attention_tokens(qkv, bias, table, 1, 7, 7, 3, 0, 0.125, pair=True),
                lambda: T.layernorm(a, torch.ones(32), torch.zeros(32), 1e-5, pair=True),
                lambda: T.patch_rows(torch.zeros(1, 8, 8, 3), pair=True),
                lambda: T.mlp(torch.zeros(4, 96), None), lambda: T.attn_block(torch.zeros(49, 96), 1, 7, 7, None, 0, 0.1),
                lambda: T.patch_embed(torch.zeros(1, 8, 8, 3), None)):
        with pytest.raises(Al3dError):
            bad()
    assert rec == []


def test_each_image_is_built_once_across_flips(rec, monkeypatch):
    from al3d import detector_ops as D, token_ops as T
    a, _, _, pk = _linear_case()
    assert rec == []                                          # nothing is packed before the first use
    for math in ("f16x3", "bf16x6", "f16x3", "bf16x6", "f32"):
        monkeypatch.setattr(D, "MATH", math)
        T.linear(a, pk)
    names = _names(rec)
    assert names.count("al3d_split_bf16x3") == 1 and names.count("al3d_split_f16x3") == 1
    assert names.count("al3d_pack_f16x3_dma") == 1
    assert [n for n in names if n.startswith("al3d_tok_")] == ["al3d_tok_linear_f16x3", "al3d_tok_linear_bf16x6",
                                                               "al3d_tok_linear_f16x3", "al3d_tok_linear_bf16x6",
                                                               "al3d_tok_linear_bf16x6"]
    assert pk.packed("bf16x6")[0] is pk.packed("bf16x6")[0]


FUSED = ("al3d_tok_attn_block_f16x3", "al3d_tok_mlp_f16x3", "al3d_tok_patch_embed_f16x3")
F16 = ("al3d_tok_linear_f16x3", "al3d_tok_window_attention_f32", "al3d_tok_window_attention_tokens_f32", "al3d_tok_mha16_f32")


def _swin_block_forward(C, heads):
    from al3d.models.swin import SwinBlock, _Geometry
    blk = SwinBlock(C, heads, 4 * C, 7, True).eval()
    x = torch.zeros(2 * 9 * 11, C)
    with torch.no_grad():
        blk(x, _Geometry.of(2, 9, 11, 7, x.device))


@pytest.mark.parametrize("math", ["bf16x6", "f32"])
@pytest.mark.parametrize("C,heads", [(96, 3), (384, 12)])
def test_swin_block_takes_the_split_bf16x6_form(rec, monkeypatch, math, C, heads):
    from al3d import detector_ops as D
    monkeypatch.setattr(D, "MATH", math)
    _swin_block_forward(C, heads)
    tok = [n for n in _names(rec) if n.startswith("al3d_tok_")]
    assert tok == ["al3d_tok_layernorm_f32", "al3d_tok_linear_bf16x6", "al3d_tok_window_attention_tokens_bf16x6",
                   "al3d_tok_linear_bf16x6", "al3d_tok_layernorm_f32", "al3d_tok_linear_bf16x6", "al3d_tok_linear_bf16x6"]
    assert not [n for n in _names(rec) if n in FUSED + F16 or "_f16x3" in n]
    ln = [args for n, args in rec if n == "al3d_tok_layernorm_f32"]
    assert [args[9] for args in ln] == [0, 0]                  # f32 rows out of both LayerNorms


def test_swin_block_keeps_its_f16x3_form(rec):
    _swin_block_forward(96, 3)
    assert [n for n in _names(rec) if n.startswith("al3d_tok_") and "image_bytes" not in n] == \
        ["al3d_tok_attn_block_f16x3", "al3d_tok_mlp_f16x3"]
    rec.clear()
    _swin_block_forward(384, 12)
    tok = [(n, args) for n, args in rec if n.startswith("al3d_tok_")]
    assert [n for n, _ in tok] == ["al3d_tok_layernorm_f32", "al3d_tok_linear_f16x3", "al3d_tok_window_attention_tokens_f32",
                                   "al3d_tok_linear_f16x3", "al3d_tok_layernorm_f32", "al3d_tok_linear_f16x3",
                                   "al3d_tok_linear_f16x3"]
    assert tok[0][1][9] == 1 and tok[1][1][1] == 1 and tok[2][1][10] == 1 and tok[5][1][14] == 1      # pair rows throughout


def _decoder_layer_forward():
    from al3d.models.transfusion_head import PositionEmbeddingLearned, TransformerDecoderLayer
    layer = TransformerDecoderLayer(128, 8, 256, self_posembed=PositionEmbeddingLearned(2, 128),
                                    cross_posembed=PositionEmbeddingLearned(2, 128)).eval()
    B, Pq, Pk = 2, 5, 40
    key_pos = torch.zeros(Pk, 2)
    with torch.no_grad():
        layer(torch.zeros(B * Pq, 128), torch.zeros(B * Pk, 128), torch.zeros(B * Pq, 2), key_pos, B)
    return layer, key_pos


@pytest.mark.parametrize("math", ["bf16x6", "f32"])
def test_transfusion_decoder_layer_runs_bf16x6(rec, monkeypatch, math):
    from al3d import detector_ops as D
    monkeypatch.setattr(D, "MATH", math)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    _decoder_layer_forward()
    names = _names(rec)
    assert names.count("al3d_tok_mha16_bf16x6") == 2 and names.count("al3d_tok_linear_bf16x6") >= 10
    assert not [n for n in names if n in FUSED + F16 or "_f16x3" in n]


def test_key_position_projection_is_cached_per_arithmetic(rec, monkeypatch):
    """The cached (key position embedding) W_kv^T rows are an activation: f16x3 rows are not served to a bf16x6 re-run, and
    flipping back computes nothing again."""
    from al3d import detector_ops as D
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    layer, key_pos = _decoder_layer_forward()
    first = layer.key_pos_projection(key_pos)
    n0 = len(rec)
    monkeypatch.setattr(D, "MATH", "bf16x6")
    second = layer.key_pos_projection(key_pos)
    assert second is not first and [n for n in _names(rec[n0:]) if n.startswith("al3d_tok_")] == ["al3d_tok_linear_bf16x6"] * 3
    n1 = len(rec)
    monkeypatch.setattr(D, "MATH", "f16x3")
    assert layer.key_pos_projection(key_pos) is first
    monkeypatch.setattr(D, "MATH", "bf16x6")
    assert layer.key_pos_projection(key_pos) is second and len(rec) == n1
