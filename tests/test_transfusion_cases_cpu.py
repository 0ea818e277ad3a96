"""CPU checks of tests/transfusion_cases.py: the float64 yardsticks against torch, the premises of the logit alphabets (what
makes an exact comparison of class and cell legitimate), the constants mirrored from the kernels, and that every case
reaches the edge it exists for.  ``pytest -s`` prints the measured gaps."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transfusion_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csrc(name):
    from al3d import lib
    return open(os.path.join(os.path.dirname(lib.__file__), "csrc", name)).read()


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).astype(np.int64)


def test_constants_mirror_the_kernels():
    src = _csrc("proposals.hip")
    assert int(re.search(r"#define TP_THREADS (\d+)", src).group(1)) == TC.TP_THREADS
    assert int(re.search(r"#define TP_MAXP (\d+)", src).group(1)) == TC.TP_MAXP
    att = _csrc("tok_attention.h")
    assert "keys_per_chunk = (int)al3d_align(al3d_cdiv(Pk, (Pk + 1023) / 1024), 32);" in att and TC.MHA_CHUNK == 1024
    assert "chunks = (int)al3d_cdiv(Pk, keys_per_chunk);" in att
    assert TC.mha16_plan(33, 1024) == (2, 1, 1024)
    assert TC.mha16_plan(33, 1025) == (2, 2, 544) and 1025 - 544 == 481
    assert TC.mha16_plan(1, 33) == (1, 1, 64) and TC.mha16_plan(32, 2049) == (1, 3, 704)
    assert TC.dominant_key("dom_chunk2", 1025) == 544 and TC.dominant_key("dom_chunk2", 33) == 32


# ------------------------------------------------------------------------------------------------------- alphabets
def test_quarter_steps_are_far_apart_in_float32():
    x = torch.arange(-32, 33, dtype=torch.float32) * 0.25
    s32 = torch.sigmoid(x).numpy()
    gap = np.diff(_bits(s32))
    own = np.abs(_bits(TC.sigmoid32(x.numpy())) - _bits(s32))
    print(f"quarter steps: {len(x)} values, least gap {gap.min()} ulp, yardstick within {own.max()} ulp of torch")
    assert len(x) == 65 and gap.min() >= 1597 and own.max() <= 2
    assert float(s32.min()) > 1e-4                                     # far from the denormal range


def test_saturation_set_is_exact_in_both_precisions():
    x = np.array([-np.inf, -200.0, -1e4, 0.0, 40.0, 1e4, np.inf], np.float32)
    want = np.array([0, 0, 0, 0.5, 1, 1, 1], np.float32)
    assert np.array_equal(torch.sigmoid(torch.from_numpy(x)).numpy(), want)
    assert np.array_equal(TC.sigmoid32(x), want)
    with np.errstate(over="ignore"):                                   # and a float32 evaluation of the kernel's expression
        assert np.array_equal(np.float32(1) / (np.float32(1) + np.exp(-x)), want)
    assert not ((x > -104) & (x < -87)).any()
    c = TC.proposal_case("saturation")
    assert set(np.unique(c["logits"]).tolist()) == set(x.tolist())


def test_fine_ladder_shares_the_high_key_bytes():
    j = np.arange(256)
    x = (j * TC.LADDER_STEP).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), j * TC.LADDER_STEP)    # exact in float32
    for s in (torch.sigmoid(torch.from_numpy(x)).numpy(), TC.sigmoid32(x)):
        b = _bits(s)
        assert np.array_equal(np.diff(b), np.full(255, 8))             # 8 ulp apart
        assert len(set((b >> 11).tolist())) == 1                       # key bits 31 .. 11 shared: passes 0 and 1 see one bin
        assert len(set(((b >> 8) & 255).tolist())) == 8 and len(set((b & 255).tolist())) == 32     # passes 2 and 3 decide
    c = TC.proposal_case("ladder")
    lad = c["logits"][0, :, :, 1].reshape(-1)
    assert np.array_equal(lad[c["cell_of_j"]], x) and np.isneginf(c["logits"][0, :, :, [0, 2]]).all()


# ------------------------------------------------------------------------------------------------------- proposals
def _torch_proposals(logits, k, free, P):
    """transfusion.py:236-275 in torch ops; a stable descending sort states the tie rule."""
    H, W, C = logits.shape
    score = torch.from_numpy(logits).permute(2, 0, 1)[None].sigmoid()
    r = k // 2
    peak = torch.zeros_like(score, dtype=torch.bool)
    peak[:, :, r:H - r, r:W - r] = score[:, :, r:H - r, r:W - r] == F.max_pool2d(score, k, 1, 0)
    for c in free:
        if c < C:
            peak[:, c] = True
    masked = (score * peak).reshape(C * H * W)
    val, top = torch.sort(masked, descending=True, stable=True)
    top = top[:P]
    return (top // (H * W)).numpy(), (top % (H * W)).numpy(), masked.reshape(C, H * W)[:, top % (H * W)].numpy(), int((masked > 0).sum())


@pytest.mark.parametrize("name", [n for n in TC.PROPOSAL_CASES if n != "workload"])
def test_proposals_ref_matches_torch(name):
    c = TC.proposal_case(name)
    for b in range(c["logits"].shape[0]):
        cls, cell, sc, npos = TC.proposals_ref(c["logits"][b], c["k"], c["free"], c["P"])
        tcls, tcell, tsc, tnpos = _torch_proposals(c["logits"][b], c["k"], c["free"], c["P"])
        assert np.array_equal(cls, tcls) and np.array_equal(cell, tcell) and npos == tnpos
        assert np.allclose(sc, tsc, rtol=0, atol=2e-7)
        assert sc.shape == (c["logits"].shape[3], c["P"]) and len(set((cls * 10 ** 6 + cell).tolist())) == c["P"]


def test_cases_reach_their_edges():
    sizes = {n: int(np.prod(TC.proposal_case(n)["logits"].shape[1:])) for n in TC.PROPOSAL_CASES}
    assert sizes["N_eq_P"] == TC.proposal_case("N_eq_P")["P"]
    assert [sizes[n] for n in ("N1023", "N1024", "N1025", "N2049")] == [TC.TP_THREADS - 1, TC.TP_THREADS, TC.TP_THREADS + 1,
                                                                         2 * TC.TP_THREADS + 1]
    assert TC.proposal_case("P256")["P"] == TC.TP_MAXP
    c = TC.proposal_case("C32")
    assert c["logits"].shape[3] == 32 and c["free"] == (31,)
    # peaks run out: fewer positive scores than proposals, and zero-score winners in ascending flat index
    for name in ("peaks_out", "k3_3x3", "k5_5x7"):
        c = TC.proposal_case(name)
        cls, cell, _, npos = TC.proposals_ref(c["logits"][0], c["k"], c["free"], c["P"])
        assert 0 < npos < c["P"], name
        rest = (cls * c["logits"].shape[1] * c["logits"].shape[2] + cell)[npos:]
        assert (np.diff(rest) > 0).all()
    assert TC.proposals_ref(TC.proposal_case("peaks_out")["logits"][0], 3, (), 200)[3] <= 90
    # constant maps
    c = TC.proposal_case("const_free")
    cls, cell, _, _ = TC.proposals_ref(c["logits"][0], c["k"], c["free"], c["P"])
    assert np.array_equal(cls * 99 + cell, np.arange(c["P"]))
    c = TC.proposal_case("const_plateau")
    cls, cell, _, npos = TC.proposals_ref(c["logits"][0], c["k"], c["free"], c["P"])
    assert npos == 7 * 9 * 10 and np.array_equal(cls, np.arange(200) // 63)
    y, x = cell // 11, cell % 11
    assert ((y >= 1) & (y < 8) & (x >= 1) & (x < 10)).all()
    # the threshold tie: `need` of 300 equal keys, the taken ones in more than one wave's share of the index range
    c = TC.proposal_case("ties_waves")
    cls, cell, _, _ = TC.proposals_ref(c["logits"][0], c["k"], c["free"], c["P"])
    flat = cls * 1024 + cell
    assert np.array_equal(flat[:100], c["above"]) and np.array_equal(flat[100:], c["tie"][:c["need"]])
    chunk = -(-sizes["ties_waves"] // TC.TP_THREADS)
    waves = np.unique(c["tie"][:c["need"]] // (64 * chunk))
    print(f"ties_waves: the {c['need']} taken ties lie in waves {waves.tolist()} of the collect step")
    assert len(waves) >= 4
    # three different samples
    c = TC.proposal_case("B3")
    assert not np.array_equal(c["logits"][0], c["logits"][1]) and not np.array_equal(c["logits"][1], c["logits"][2])


def test_nan_case_places_nan_where_a_cell_may_propose():
    c, nan_flat = TC.nan_case()
    masked = TC.masked_scores(c["logits"][0], c["k"], c["free"]).reshape(-1)
    assert np.array_equal(np.flatnonzero(np.isnan(masked)), nan_flat) and len(nan_flat) == 5
    # torch's descending argsort puts NaN first
    top = torch.from_numpy(masked).argsort(descending=True)[:5]
    assert sorted(top.tolist()) == nan_flat.tolist()


# ------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("regime", ("random",) + TC.MHA_REGIMES)
@pytest.mark.parametrize("B,Pq,Pk,heads", [(1, 5, 33, 3), (2, 33, 1025, 1)])
def test_mha16_ref_matches_torch(B, Pq, Pk, heads, regime):
    q, k, v = TC.mha_case(regime, B, Pq, Pk, heads)
    ref, ref32 = TC.mha16_ref(q, k, v, B, Pq, Pk, heads, 0.25)

    def hf(x, L):
        return torch.from_numpy(x).double().reshape(B, L, heads, 16).permute(0, 2, 1, 3)
    want = F.scaled_dot_product_attention(hf(q, Pq), hf(k, Pk), hf(v, Pk), scale=0.25).permute(0, 2, 1, 3).reshape(B * Pq, -1)
    assert ref.dtype == np.float64 and ref32.dtype == np.float32
    assert float(np.abs(ref - want.numpy()).max()) <= 1e-12
    assert float(np.abs(ref32 - ref).max()) <= 1e-5
    vv = v.astype(np.float64).reshape(B, Pk, heads * 16)
    if regime == "k0":                                                  # the mean of v over exactly Pk keys
        assert float(np.abs(ref.reshape(B, Pq, -1) - vv.mean(1, keepdims=True)).max()) <= 1e-13
        # a padding key counted once would scale the result by Pk / (Pk + 1): far outside the GPU test's bound
        assert float(np.abs(vv.mean(1)).max()) / (Pk + 1) > 1e-5
    if regime.startswith("dom_"):
        key = TC.dominant_key(regime, Pk)
        assert float(np.abs(ref.reshape(B, Pq, -1) - vv[:, key:key + 1]).max()) <= 1e-12
        lg = (q.astype(np.float64)[:Pq, :16] * 0.25) @ k.astype(np.float64)[:Pk, :16].T
        assert float((lg[:, key] - np.delete(lg, key, axis=1).max(1)).min()) > 50.0
    if regime in ("rising", "falling"):
        lg = (q.astype(np.float64)[:Pq, :16] * 0.25) @ k.astype(np.float64)[:Pk, :16].T
        tile_max = np.array([lg[:, t:t + 32].max(1) for t in range(0, Pk, 32)])          # [tiles, Pq]
        d = np.diff(tile_max, axis=0)
        assert (d > 0).all() if regime == "rising" else (d < 0).all()
