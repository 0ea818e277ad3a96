"""CPU suite: the C oracle against the numpy / torch yardstick (tests/selector_numpy.py) at NaN,
inf, signed zeros and the other edge cases of tests/selector_edge_cases.py.

The oracle and the HIP kernels were written by one hand; the yardstick is made from the calls the
reference itself makes, so a shared misreading of ``argmax`` / ``min(0)`` / ``argsort`` shows here
without a GPU."""
import numpy as np
import pytest
import torch

import selector_edge_cases as C
import selector_numpy as Y


@pytest.mark.parametrize("dtype", C.GREEDY_DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", C.GREEDY_N)
def test_oracle_greedy_edges(oracle, n, dtype):
    for label, D, box, runs in C.greedy_cases(n, dtype):
        for run in runs:
            for budget in C.GREEDY_BUDGETS:
                ref = Y.greedy(D, run["seeded"], run["first"], box, C.COST_F, C.START_COST, budget,
                               check_seeded=run["check_seeded"])
                rc, picks = oracle.greedy(D, run["seeded"], run["first"], box, C.COST_F, C.START_COST,
                                          budget, check_seeded=run["check_seeded"])
                assert (rc, picks.tolist()) == ref, (label, run, budget)


def test_issue_example_nan_frame(oracle):
    """n = 40, frame 7 NaN, frame 3 seeded: the reference loop picks [7, 0] and then asserts."""
    rng = np.random.default_rng(0)
    D = rng.uniform(0.5, 4.0, size=(40, 40)).astype(np.float32)
    D = np.minimum(D, D.T)
    np.fill_diagonal(D, 0)
    D[7, :] = np.nan
    D[:, 7] = np.nan
    box = np.zeros(40)
    assert Y.greedy(D, [3], -1, box, 0.12, 0.0, 1.0) == (-1, [7, 0])
    rc, picks = oracle.greedy(D, [3], -1, box, 0.12, 0.0, 1.0)
    assert (rc, picks.tolist()) == (-1, [7, 0])


def test_yardstick_cap_and_seed_map(oracle):
    """The two arguments the edge list does not vary: ``cap`` (-2) and a separate ``seed_map``."""
    D, box = C._greedy_base(70, np.float64)
    S = np.ascontiguousarray(D[::-1, ::-1])
    for kw in (dict(cap=4), dict(seed_map=S), dict(seed_map=S, cap=1)):
        ref = Y.greedy(D, [5, 9], -1, box, 0.12, 0.0, 60.0, **kw)
        rc, picks = oracle.greedy(D, [5, 9], -1, box, 0.12, 0.0, 60.0, **kw)
        assert (rc, picks.tolist()) == ref, kw
    assert Y.greedy(D, [5, 9], -1, box, 0.12, 0.0, 60.0, cap=4)[0] == -2


@pytest.mark.parametrize("kind", C.ARGSORT_KINDS)
@pytest.mark.parametrize("n", C.ARGSORT_N)
def test_argsort_key_formula(oracle, kind, n):
    """The kernel's key formula (csrc/al3d_sort_key.h, evaluated on the CPU): sorting the keys in
    descending order must give torch's and numpy's stable argsort of -x."""
    x = C.argsort_input(kind, n)
    ref = Y.argsort_desc(x)
    assert np.array_equal(ref, Y.argsort_desc_numpy(x)), "torch and numpy disagree"
    keys = oracle.sort_keys(x)
    assert np.unique(keys).size == n
    assert np.array_equal(np.argsort(keys)[::-1], ref)
    assert np.array_equal(oracle.argsort_desc(x), ref)


def test_argsort_key_formula_issue_example(oracle):
    x = np.array([-0.0, 0.0, 1.0, -0.0, 0.0], dtype=np.float32)
    assert Y.argsort_desc(x).tolist() == [2, 0, 1, 3, 4]
    assert np.argsort(oracle.sort_keys(x))[::-1].tolist() == [2, 0, 1, 3, 4]


def test_oracle_frame_entropy_edges(oracle):
    scores, _, counts, _ = C.entropy_inputs()
    ref = Y.frame_entropy(scores, counts)
    got = np.array([oracle.frame_entropy(np.concatenate([scores[b, t, :counts[b, t]] for t in range(2)]))
                    for b in range(scores.shape[0])], dtype=np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.isnan(ref).sum() == 3                  # the empty frame and the scores of 0 and 1
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=2e-6, atol=0)


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("n,c", C.L1_SHAPES)
def test_oracle_l1_map_non_finite(oracle, n, c, p):
    f = C.l1_input(n, c)
    ref = Y.l1_map(f, p)
    got = oracle.l1_map_f32(f, p)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and not np.isneginf(got).any()
    assert np.isnan(ref[9, 66]) and np.isposinf(ref[9, 10]) and np.isnan(ref[4]).all()
    fin = np.isfinite(ref)
    # torch's vectorised reduction order differs from the oracle's (tests/test_oracle_golden.py)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=2e-6, atol=0)


@pytest.mark.parametrize("n", [1, 257])
def test_oracle_euclid_map(oracle, n):
    xy, loc = C.euclid_input(n)
    ref = Y.euclid_map(xy, loc)
    got = oracle.euclid_map(xy, loc)
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))
    if n > 10:
        assert ref[1, 3] == 0.0 and ref[1, 8] == 1e6


def test_yardstick_matches_torch_on_the_documented_examples():
    """Guards the yardstick itself: the facts about numpy / torch the fixes rest on."""
    nan = float("nan")
    assert int(torch.argmax(torch.tensor([1.0, nan, 5.0, nan]))) == 1
    assert int(np.argmax(np.array([1.0, nan, 5.0, nan]))) == 1
    m = torch.stack([torch.tensor([1.0, nan, 2.0]), torch.tensor([nan, 0.0, 1.0])]).min(0)[0]
    assert torch.isnan(m[:2]).all() and m[2] == 1.0
    m = np.stack([np.array([1.0, nan, 2.0]), np.array([nan, 0.0, 1.0])]).min(0)
    assert np.isnan(m[:2]).all() and m[2] == 1.0
