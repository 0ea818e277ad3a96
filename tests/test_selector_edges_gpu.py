"""GPU suite: the HIP selection kernels against the numpy / torch yardstick
(tests/selector_numpy.py) at NaN, inf, signed zeros and at every size where a kernel takes
another path (tests/selector_edge_cases.py).  tests/test_selector_gpu.py pins the same kernels to
the C oracle on finite input; this file pins them to what numpy and torch themselves do."""
import numpy as np
import pytest
import torch

import selector_edge_cases as C
import selector_numpy as Y

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import hip_backend
    return hip_backend


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from al3d import selector_ops
    return selector_ops


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- greedy
@pytest.mark.parametrize("dtype", C.GREEDY_DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", C.GREEDY_N)
def test_greedy_edges(ops, n, dtype):
    for label, D, box, runs in C.greedy_cases(n, dtype):
        Dd, boxd = _d(D), _d(box)                    # one upload per map
        for run in runs:
            for budget in C.GREEDY_BUDGETS:
                ref = Y.greedy(D, run["seeded"], run["first"], box, C.COST_F, C.START_COST, budget,
                               check_seeded=run["check_seeded"])
                got = ops.greedy_kcenter(Dd, run["seeded"], run["first"], boxd, C.COST_F, C.START_COST,
                                         budget, check_seeded=run["check_seeded"])
                assert got == ref, (label, run, budget)
                if label == "ppal_neg_inf" and budget == 60.0:
                    assert ref[0] == -1              # the reference runs into its assert


def test_greedy_issue_example_through_backend(hip):
    """n = 40, frame 7 NaN, frame 3 seeded: the reference loop picks [7, 0] and then asserts."""
    rng = np.random.default_rng(0)
    D = rng.uniform(0.5, 4.0, size=(40, 40)).astype(np.float32)
    D = np.minimum(D, D.T)
    np.fill_diagonal(D, 0)
    D[7, :] = np.nan
    D[:, 7] = np.nan
    rc, picks = hip.greedy(D, [3], -1, np.zeros(40), 0.12, 0.0, 1.0)
    assert (rc, picks.tolist()) == (-1, [7, 0]) == Y.greedy(D, [3], -1, np.zeros(40), 0.12, 0.0, 1.0)


# ---------------------------------------------------------------- argsort
@pytest.mark.parametrize("n", C.ARGSORT_N)
def test_argsort_desc_edges(hip, n):
    for kind in C.ARGSORT_KINDS:
        x = C.argsort_input(kind, n)
        got = hip.argsort_desc(x)
        assert np.array_equal(got, Y.argsort_desc(x)), kind
        assert np.array_equal(got, Y.argsort_desc_numpy(x)), kind


# ---------------------------------------------------------------- minmax
@pytest.mark.parametrize("n", C.MINMAX_N)
def test_minmax_norm_edges(ops, n):
    for label, x in C.minmax_inputs(n):
        ref = Y.minmax_norm(x)
        got = ops.minmax_norm(_d(x)).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref)), label
        assert np.array_equal(np.isinf(got), np.isinf(ref)), label
        assert np.array_equal(np.signbit(got[np.isinf(ref)]), np.signbit(ref[np.isinf(ref)])), label
        fin = np.isfinite(ref)
        np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-6, atol=0, err_msg=label)
        if label == "constant" or n == 1:
            assert np.isnan(ref).all()
        if label == "extremes_third_pass":
            assert got[2048] == 0.0 and got[n - 1] == 1.0


# ---------------------------------------------------------------- scale_rows
@pytest.mark.parametrize("c", [1, 7, 512])
def test_scale_rows_edges(ops, c):
    rng = np.random.default_rng(c)
    n, m = 301, 40
    f = rng.normal(size=(n, c)).astype(np.float32)
    f[2, 0] = 0.0                                    # 0 * inf = NaN
    for weights in ("finite", "non_finite"):
        w = rng.uniform(size=n).astype(np.float32)
        wm = rng.uniform(size=m).astype(np.float32)
        if weights == "non_finite":
            w[[1, 2, 3, 300]] = [np.nan, np.inf, -np.inf, np.nan]
            wm[[0, 1, 39]] = [np.nan, np.inf, -np.inf]
        got = ops.scale_rows(_d(f), _d(w)).cpu().numpy()
        assert np.array_equal(got, Y.scale_rows(f, w), equal_nan=True), weights
        perm = rng.permutation(n).astype(np.int64)
        got = ops.scale_rows(_d(f), _d(w), _d(perm)).cpu().numpy()
        assert np.array_equal(got, Y.scale_rows(f, w, perm), equal_nan=True), weights
        rep = rng.integers(0, m, size=n).astype(np.int64)      # repeats, weight vector shorter than n
        rep[:3] = [0, 1, 39]
        got = ops.scale_rows(_d(f), _d(wm), _d(rep)).cpu().numpy()
        assert np.array_equal(got, Y.scale_rows(f, wm, rep), equal_nan=True), weights


# ---------------------------------------------------------------- frame entropy
def test_frame_entropy_edges(ops):
    """Tolerances of the existing tests, relative to torch float32; the NaN pattern is exact.  A
    label outside [0, ncls) is not tried inside the counts: the reference raises IndexError
    there and the kernel weights the box 0 (include/al3d.h)."""
    scores, labels, counts, cw = C.entropy_inputs()
    ref = Y.frame_entropy(scores, counts)
    got = ops.frame_entropy(_d(scores), _d(counts)).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.isnan(ref).tolist() == [True] + [False] * 7 + [True, True, False]
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=2e-6, atol=0)
    ref = Y.frame_weighted_entropy(scores, labels, counts, cw)
    got = ops.frame_weighted_entropy(_d(scores), _d(labels), _d(counts), _d(cw)).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.isnan(ref).tolist() == [False] * 8 + [True, True, False] and ref[0] == 0.0 == got[0]
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-5, atol=0)


# ---------------------------------------------------------------- mask map
@pytest.mark.parametrize("n", [1, 300])
def test_mask_map_edges(ops, n):
    rng = np.random.default_rng(n)
    D = rng.uniform(0, 5, size=(n, n)).astype(np.float32)
    for keep in (np.ones(n, bool), np.zeros(n, bool), rng.uniform(size=n) < 0.4):
        got = ops.mask_map_(_d(D), _d(keep.astype(np.uint8))).cpu().numpy()
        assert np.array_equal(got, Y.mask_map(D, keep))


def test_mask_map_clamped_grid(ops):
    """n = 16640 is 65 column blocks, one more than the grid's 64: the stride loop runs.  The map
    is 1.1 GB, so it is compared on the device."""
    n = 16640
    g = torch.Generator(device=DEV).manual_seed(0)
    D = torch.rand((n, n), generator=g, device=DEV, dtype=torch.float32)
    rnd = torch.rand(n, generator=g, device=DEV) < 0.4
    rnd[n - 1] = True
    rnd[16384] = False
    neg = torch.tensor(-float("inf"), device=DEV)
    for keep in (torch.ones(n, dtype=torch.bool, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV), rnd):
        got = ops.mask_map_(D.clone(), keep.to(torch.uint8))
        ref = torch.where(keep[:, None] & keep[None, :], D, neg)
        assert torch.equal(got, ref)
        del got, ref


# ---------------------------------------------------------------- L1 map
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("n,c", C.L1_SHAPES)
def test_l1_map_non_finite(hip, oracle, n, c, p):
    f = C.l1_input(n, c)
    ref = Y.l1_map(f, p)
    got = hip.l1_map_f32(f, p)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and not np.isneginf(got).any()
    fin = np.isfinite(ref)
    orc = oracle.l1_map_f32(f, p)                    # finite entries: the existing bit-exact contract
    assert np.array_equal(got[fin].view(np.int32), orc[fin].view(np.int32))


# ---------------------------------------------------------------- Euclid map
@pytest.mark.parametrize("n", [1, 257])
def test_euclid_map_direct(hip, n):
    xy, loc = C.euclid_input(n)
    ref = Y.euclid_map(xy, loc)
    got = hip.euclid_map(xy, loc)
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))
