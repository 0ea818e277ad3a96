"""GPU suite: the TransFusion head's own device kernels at their edges, against the float64 yardsticks of
tests/transfusion_cases.py (whose premises tests/test_transfusion_cases_cpu.py asserts).

Proposals (csrc/proposals.hip): class and cell compare with ``array_equal`` -- every case draws its logits from an alphabet
on which the order of the float32 scores does not depend on the sigmoid's last bits; masked scores to 2e-7; query positions
and features exactly (gathers and two float32 additions in the kernel's order).

mha16 (tok_mha16_kernel + tok_mha16_combine_kernel), under both arithmetics: e <= 3 e32 + 1e-6 against ``mha16_ref`` (e32:
torch's float32 evaluation of the same expression), and e <= 1e-5 where the logits are O(1); the known-answer regimes add
their own statements.  ``pytest -s`` prints e and e32 per case."""
import contextlib

import numpy as np
import pytest
import torch

import transfusion_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_I, SENT_F = -7, -12345.0


# ------------------------------------------------------------------------------------------------------- proposals
def _run_proposals(logits, k, free, P, hidden=8, sizes=None, refused=False):
    """Calls al3d_tf_proposals_f32 on sentinel-filled outputs.  ``sizes`` = (B, H, W, C) overrides what the entry is told (the
    refusal tests); the buffers are then sized for the larger of both.  ``refused``: the call must raise Al3dError; the outputs
    are returned as the refused call left them."""
    from al3d import lib
    from al3d.selector_ops import _ptr, _stream
    B, H, W, C = sizes or logits.shape
    ab, ah, aw, ac = (max(a, b, 1) for a, b in zip((B, H, W, C), logits.shape))
    g = torch.Generator().manual_seed(5)
    tokens = torch.randn(ab * ah * aw, hidden, generator=g)
    bev_pos = torch.rand(ah * aw, 2, generator=g) * 30
    cols, bias = torch.randn(ac, hidden, generator=g), torch.randn(hidden, generator=g)
    ap = max(P, 1)
    out = dict(cls=torch.full((ab, ap), SENT_I, dtype=torch.int64, device=DEV),
               cell=torch.full((ab, ap), SENT_I, dtype=torch.int64, device=DEV),
               score=torch.full((ab, ac, ap), SENT_F, device=DEV), feat=torch.full((ab * ap, hidden), SENT_F, device=DEV),
               pos=torch.full((ab * ap, 2), SENT_F, device=DEV))
    ws = torch.empty(max(int(lib.load().al3d_tf_proposals_workspace_bytes(ab, ah, aw, ac)), 256), dtype=torch.uint8, device=DEV)
    dev = [t.to(DEV).contiguous() for t in (torch.from_numpy(np.ascontiguousarray(logits)), tokens, bev_pos, cols, bias)]
    try:
        with pytest.raises(lib.Al3dError) if refused else contextlib.nullcontext():
            lib.call("al3d_tf_proposals_f32", _ptr(dev[0]), B, H, W, C, k, sum(1 << c for c in free if c < 32), P, _ptr(dev[1]), hidden,
                     _ptr(dev[2]), _ptr(dev[3]), _ptr(dev[4]), _ptr(ws), _ptr(out["cls"]), _ptr(out["cell"]), _ptr(out["score"]),
                     _ptr(out["feat"]), _ptr(out["pos"]), _stream())
    finally:
        torch.cuda.synchronize()
        out = {n: t.cpu() for n, t in out.items()}
    return out, dict(tokens=tokens, bev_pos=bev_pos, cols=cols, bias=bias)


def _untouched(out):
    return all(bool((out[n] == (SENT_I if n in ("cls", "cell") else SENT_F)).all()) for n in out)


@pytest.mark.parametrize("name", TC.PROPOSAL_CASES)
def test_proposals_match_the_yardstick_exactly(name):
    c = TC.proposal_case(name)
    logits, k, free, P = c["logits"], c["k"], c["free"], c["P"]
    B, H, W, C = logits.shape
    out, inp = _run_proposals(logits, k, free, P)
    hidden = inp["tokens"].shape[1]
    pos, feat = out["pos"].view(B, P, 2), out["feat"].view(B, P, hidden)
    for b in range(B):
        got_cls, got_cell, got_sc = out["cls"][b].numpy(), out["cell"][b].numpy(), out["score"][b].numpy()
        flat = got_cls * (H * W) + got_cell
        if name == "ladder":
            # the premise, on the kernel's own scores: they increase strictly with j.  If this fails the ladder is too fine
            # for the device's sigmoid (double LADDER_STEP), not the selection wrong
            j_of_cell = np.empty(H * W, np.int64)
            j_of_cell[c["cell_of_j"]] = np.arange(H * W)
            assert (got_cls == 1).all() and len(set(got_cell.tolist())) == P
            by_j = np.argsort(j_of_cell[got_cell])
            assert (np.diff(got_sc[1, by_j]) > 0).all(), "premise: the device sigmoid does not separate the ladder"
        cls, cell, sc, npos = TC.proposals_ref(logits[b], k, free, P)
        assert np.array_equal(got_cls, cls), (name, b)
        assert np.array_equal(got_cell, cell), (name, b)
        assert np.allclose(got_sc, sc, rtol=0, atol=2e-7)
        assert len(set(flat.tolist())) == P
        assert torch.equal(pos[b], inp["bev_pos"][out["cell"][b]])
        assert torch.equal(feat[b], inp["tokens"][b * H * W + out["cell"][b]] + (inp["cols"][out["cls"][b]] + inp["bias"]))
        own = got_sc[got_cls, np.arange(P)]                          # each winner's own masked score
        if name == "const_free":
            assert np.array_equal(flat, np.arange(P))
        if name == "const_plateau":
            assert (own > 0).all() and (np.diff(flat) > 0).all()
        if name == "ties_waves":
            assert np.array_equal(flat[100:], c["tie"][:c["need"]])
        if name == "ladder":
            assert np.array_equal(got_cell, c["cell_of_j"][::-1][:P])
        if name in ("peaks_out", "k3_3x3", "k5_5x7", "N_eq_P"):
            # the peaks run out: the positive winners are the yardstick's, the rest are zero-score cells in ascending flat index
            assert npos < P and (name != "peaks_out" or npos <= 90)
            assert (own[:npos] > 0).all() and (own[npos:] == 0).all() and (np.diff(flat[npos:]) > 0).all()
        if name == "saturation":
            assert set(np.unique(got_sc).tolist()) <= {0.0, 0.5, 1.0}


def test_proposals_nan_logits_stay_in_range_and_come_first():
    """The contract written at the top of csrc/proposals.hip: a NaN score at a cell that may propose sorts before every
    finite score, as torch's descending argsort puts it; every output stays in range and the winners stay distinct."""
    c, nan_flat = TC.nan_case()
    B, H, W, C = c["logits"].shape
    out, _ = _run_proposals(c["logits"], c["k"], c["free"], c["P"])
    cls, cell = out["cls"][0].numpy(), out["cell"][0].numpy()
    assert ((cls >= 0) & (cls < C)).all() and ((cell >= 0) & (cell < H * W)).all()
    flat = cls * (H * W) + cell
    assert len(set(flat.tolist())) == c["P"]
    assert sorted(flat[:len(nan_flat)].tolist()) == nan_flat.tolist()
    own = out["score"][0].numpy()[cls, np.arange(c["P"])]
    assert np.isnan(own[:len(nan_flat)]).all() and not np.isnan(own[len(nan_flat):]).any()
    assert (np.diff(own[len(nan_flat):]) <= 0).all()
    assert bool(torch.isfinite(out["pos"]).all()) and bool(torch.isfinite(out["feat"]).all())


def test_proposals_of_an_empty_batch_touch_nothing():
    c = TC.proposal_case("P200")
    out, _ = _run_proposals(c["logits"], c["k"], c["free"], c["P"], sizes=(0,) + c["logits"].shape[1:])
    assert _untouched(out)


@pytest.mark.parametrize("what,sizes,k,P", [
    ("P0", (1, 9, 11, 10), 3, 0), ("P257", (1, 9, 11, 10), 3, 257), ("C0", (1, 9, 11, 0), 3, 200), ("C33", (1, 9, 11, 33), 3, 200),
    ("k2", (1, 9, 11, 10), 2, 200), ("k4", (1, 9, 11, 10), 4, 200), ("k0", (1, 9, 11, 10), 0, 200),
    ("k7_on_3_rows", (1, 3, 40, 10), 7, 200), ("k7_on_3_columns", (1, 40, 3, 10), 7, 200), ("N_below_P", (1, 3, 3, 10), 3, 200)])
def test_proposals_refusals_leave_the_outputs_alone(what, sizes, k, P):
    logits = np.zeros(sizes[:3] + (max(sizes[3], 1),), np.float32)
    out, _ = _run_proposals(logits, k, (8, 9), P, sizes=sizes, refused=True)
    assert _untouched(out), what


# ------------------------------------------------------------------------------------------------------- mha16
@pytest.fixture(params=["f16x3", "bf16x6"])
def arith(request, monkeypatch):
    from al3d import detector_ops as D
    monkeypatch.setattr(D, "MATH", request.param)
    return request.param


def _embed(x, col, pitch, seed):
    """x as a column slice starting at ``col`` of a device matrix of row pitch ``pitch`` filled with other numbers."""
    m = torch.randn(x.shape[0], pitch, generator=torch.Generator().manual_seed(seed)) * 50.0
    m[:, col:col + x.shape[1]] = torch.from_numpy(x)
    return m.to(DEV)[:, col:col + x.shape[1]]


def _mha(regime, B, Pq, Pk, heads, sliced=False):
    from al3d import token_ops as T
    q, k, v = TC.mha_case(regime, B, Pq, Pk, heads)
    ref, ref32 = TC.mha16_ref(q, k, v, B, Pq, Pk, heads, 0.25)
    C = heads * 16
    if sliced:
        # q and k at column offset 4 of wider matrices; v from an odd column of a matrix with an odd pitch (only q and k
        # carry alignment rules)
        dq, dk, dv = _embed(q, 4, C + 8, 1), _embed(k, 4, C + 12, 2), _embed(v, 1, C + 3, 3)
        assert dv.stride(0) % 2 == 1 and dv.storage_offset() == 1 and dq.storage_offset() == 4
    else:
        dq, dk, dv = (torch.from_numpy(t).to(DEV) for t in (q, k, v))
    got = T.mha16(dq, dk, dv, B, Pq, Pk, heads, 0.25).cpu().numpy()
    return got, ref, ref32, v


def _bound(tag, got, ref, ref32, unit_logits):
    e, e32 = float(np.abs(got - ref).max()), float(np.abs(ref32 - ref).max())
    print(f"mha16 {tag}: e={e:.3e} e32={e32:.3e}")
    assert np.isfinite(got).all()
    assert e <= 3.0 * e32 + 1e-6, (tag, e, e32)
    if unit_logits:
        assert e <= 1e-5, (tag, e)


SHAPES = ([(1, pq, pk, 8) for pq in (1, 31, 32, 33) for pk in (1, 31, 32, 33)] +
          [(1, 33, pk, 8) for pk in (1023, 1024, 1025, 2049)] +
          [(1, 33, pk, h) for pk in (33, 1025) for h in (1, 3)] + [(2, 33, 33, 3), (2, 33, 1025, 8)])


@pytest.mark.parametrize("B,Pq,Pk,heads", SHAPES)
def test_mha16_shape_edges(arith, B, Pq, Pk, heads):
    got, ref, ref32, _ = _mha("random", B, Pq, Pk, heads)
    _bound(f"{arith} random B={B} Pq={Pq} Pk={Pk} heads={heads}", got, ref, ref32, True)


@pytest.mark.parametrize("B,Pq,Pk,heads", [(1, 5, 33, 8), (2, 33, 1025, 3)])
def test_mha16_odd_v_layout_and_offset_q_k(arith, B, Pq, Pk, heads):
    got, ref, ref32, _ = _mha("random", B, Pq, Pk, heads, sliced=True)
    _bound(f"{arith} sliced B={B} Pq={Pq} Pk={Pk} heads={heads}", got, ref, ref32, True)


@pytest.mark.parametrize("Pk", [33, 1025])
@pytest.mark.parametrize("regime", TC.MHA_REGIMES)
def test_mha16_known_answers(arith, regime, Pk):
    B, Pq, heads = 2, 33, 3
    got, ref, ref32, v = _mha(regime, B, Pq, Pk, heads)
    _bound(f"{arith} {regime} B={B} Pq={Pq} Pk={Pk} heads={heads}", got, ref, ref32, regime == "k0")
    vv = v.astype(np.float64).reshape(B, Pk, heads * 16)
    out = got.astype(np.float64).reshape(B, Pq, heads * 16)
    if regime == "k0":
        # uniform weights over exactly Pk keys; one padding key counted would cost a factor Pk / (Pk + 1)
        mean = vv.mean(1, keepdims=True)
        e32 = float(np.abs(ref32 - ref).max())
        assert float(np.abs(out - mean).max()) <= 3.0 * e32 + 1e-6
        assert float(np.abs(mean).max()) / (Pk + 1) > 10.0 * (3.0 * e32 + 1e-6)        # the bound sees that factor
    if regime.startswith("dom_"):
        key = TC.dominant_key(regime, Pk)
        assert float(np.abs(out - vv[:, key:key + 1]).max()) <= 1e-6 * float(np.abs(v).max())


def test_mha16_writes_stay_inside_output_block_and_workspace(arith):
    """The C entry with a wide output pitch, two spare output rows and 4 KB behind the stated workspace, all sentinel-filled:
    the partials of the padded query rows (Pq = 33: 31 of them per tile pair) and of the short last chunk stay inside."""
    from al3d import lib
    from al3d import token_ops as T
    B, Pq, Pk, heads = 2, 33, 1025, 3
    C, ldo = heads * 16, heads * 16 + 8
    q, k, v = (torch.from_numpy(t).to(DEV) for t in TC.mha_case("random", B, Pq, Pk, heads))
    want = T.mha16(q, k, v, B, Pq, Pk, heads, 0.25)
    nbytes = int(lib.load().al3d_tok_mha16_workspace_bytes(B, heads, Pq, Pk))
    qtiles, chunks, _ = TC.mha16_plan(Pq, Pk)
    assert nbytes == -(-B * heads * chunks * qtiles * 32 * 18 * 4 // 256) * 256
    out = torch.full((B * Pq + 2, ldo), SENT_F, device=DEV)
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    lib.call("al3d_tok_mha16_f32" if arith == "f16x3" else "al3d_tok_mha16_bf16x6", q.data_ptr(), q.stride(0), k.data_ptr(),
             k.stride(0), v.data_ptr(), v.stride(0), B, heads, Pq, Pk, 0.25, out.data_ptr(), ldo, ws.data_ptr(),
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out[:B * Pq, :C], want)
    assert bool((out[:B * Pq, C:] == SENT_F).all()) and bool((out[B * Pq:] == SENT_F).all())
    assert bool((ws[nbytes:] == 0xA5).all())


def test_mha16_refusals(arith):
    from al3d import token_ops as T
    from al3d.lib import Al3dError
    B, Pq, Pk, heads, C = 1, 5, 33, 3, 48
    z = lambda r, c: torch.zeros(r, c, device=DEV)                    # noqa: E731
    q, k, v = z(Pq, C), z(Pk, C), z(Pk, C)
    T.mha16(q, k, v, B, Pq, Pk, heads, 0.25)                          # the accepted form of what follows
    with pytest.raises(Al3dError):
        T.mha16(z(Pq, C + 2)[:, :C], k, v, B, Pq, Pk, heads, 0.25)    # q pitch no multiple of 4
    with pytest.raises(Al3dError):
        T.mha16(q, z(Pk, C + 2)[:, :C], v, B, Pq, Pk, heads, 0.25)    # k pitch no multiple of 4
    with pytest.raises(Al3dError):
        T.mha16(z(Pq, C + 4)[:, 2:C + 2], k, v, B, Pq, Pk, heads, 0.25)      # q base 8 bytes off
    with pytest.raises(Al3dError):
        T.mha16(q, z(Pk, C + 4)[:, 1:C + 1], v, B, Pq, Pk, heads, 0.25)      # k base 4 bytes off
    with pytest.raises(Al3dError):
        T.mha16(z(Pq, C - 16), k, v, B, Pq, Pk, heads, 0.25)          # q pitch < heads * 16
    with pytest.raises(Al3dError):
        T.mha16(q, k, z(Pk, C - 16), B, Pq, Pk, heads, 0.25)          # v pitch < heads * 16
    with pytest.raises(Al3dError):
        T.mha16(q, z(0, C), z(0, C), B, Pq, 0, heads, 0.25)           # Pk = 0
