"""The edge-case inputs shared by tests/test_selector_edges_cpu.py (C oracle against the numpy /
torch yardstick) and tests/test_selector_edges_gpu.py (HIP kernels against the same yardstick).

Only inputs are built here; every expectation comes from tests/selector_numpy.py.
"""
import functools

import numpy as np

GREEDY_N = (70, 1030, 2100)        # 1024 threads: a partial first pass, a second pass, a third
GREEDY_DTYPES = (np.float64, np.float32)
GREEDY_BUDGETS = (3.0, 60.0)
COST_F, START_COST = 0.12, 0.37


@functools.lru_cache(maxsize=None)
def _greedy_base(n, dtype):
    rng = np.random.default_rng(n)
    # quantised values => plenty of exact ties for the first-index rule
    D = (rng.integers(1, 40, size=(n, n)) / 8.0).astype(dtype)
    D = np.minimum(D, D.T)
    np.fill_diagonal(D, 0)
    box = rng.integers(0, 70, size=n) * 0.04
    return D, box


def _run(seeded=(), first=-1, check_seeded=False):
    return dict(seeded=list(seeded), first=first, check_seeded=check_seeded)


def _others(n, rng, k, exclude):
    pool = np.setdiff1d(np.arange(n), np.asarray(exclude))
    return sorted(int(v) for v in rng.choice(pool, size=k, replace=False))


def greedy_cases(n, dtype):
    """Yield ``(label, D, box_cost, runs)``; every run is tried at every budget."""
    D0, box = _greedy_base(n, dtype)
    rng = np.random.default_rng(1000 + n)
    # one whole row + column NaN: the frame without a surviving box under Badge / UWE
    for p in (0, 5, 64, 1029):
        if p >= n:
            continue
        D = D0.copy()
        D[p, :] = np.nan
        D[:, p] = np.nan
        q = (p + 3) % n
        out = _others(n, rng, 3, [p])
        ins = sorted(out[:2] + [p])
        runs = [_run(first=p), _run(first=q)]
        for cs in (False, True):
            runs += [_run(seeded=out, check_seeded=cs), _run(seeded=ins, check_seeded=cs)]
        yield f"nan_row{p}", D, box, runs
    # one NaN entry only, in a row the loop starts from and in a column of the last pass
    D = D0.copy()
    a, b = 3, n - 2
    D[a, b] = np.nan
    yield "nan_entry", D, box, [_run(first=a), _run(first=b), _run(first=7),
                                _run(seeded=[a, 11]), _run(seeded=[11, 12], check_seeded=True)]
    # +inf entries: a disconnected spatial map under normalize="none"
    D = D0.copy()
    comp = rng.integers(0, 3, size=n)
    D[comp[:, None] != comp[None, :]] = np.inf
    yield "pos_inf", D, box, [_run(first=0), _run(first=n - 1), _run(seeded=_others(n, rng, 3, [])),
                              _run(seeded=_others(n, rng, 2, []), check_seeded=True)]
    # PPAL: -inf outside a kept set of 3 frames, budget larger than the kept set
    D = D0.copy()
    kept = np.array(_others(n, rng, 2, [n - 1]) + [n - 1])
    keep = np.zeros(n, dtype=bool)
    keep[kept] = True
    D[~keep] = -np.inf
    D[:, ~keep] = -np.inf
    yield "ppal_neg_inf", D, np.zeros(n), [_run(seeded=[int(kept[0])]), _run(seeded=[int(kept[2])]),
                                           _run(seeded=[int(kept[0]), int(kept[1])])]


# ---------------------------------------------------------------- argsort
ARGSORT_N = (1, 2, 3, 1023, 1024, 1025, 2049)
ARGSORT_KINDS = ("signed_zeros", "all_equal", "all_nan", "negative_nan", "inf", "subnormal",
                 "ascending", "descending")


def argsort_input(kind, n):
    rng = np.random.default_rng(n)
    if kind == "signed_zeros":
        x = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], dtype=np.float32), size=n)
        x[0] = -0.0
        return x
    if kind == "all_equal":
        return np.full(n, 0.25, dtype=np.float32)
    if kind == "all_nan":
        return np.full(n, np.nan, dtype=np.float32)
    if kind == "negative_nan":
        x = rng.normal(size=n).astype(np.float32)
        bits = x.view(np.uint32)
        bits[::3] = 0xffc00000                      # NaN with the sign bit set
        bits[1::7] = 0x7fc00000
        return x
    if kind == "inf":
        return rng.choice(np.array([np.inf, -np.inf, 0.5, -2.0, 3e38], dtype=np.float32), size=n)
    if kind == "subnormal":
        x = (rng.integers(-6, 7, size=n).astype(np.float32) * np.float32(1e-45))
        return x
    if kind == "ascending":
        return np.arange(n, dtype=np.float32) / 8 - 3
    if kind == "descending":
        return -np.arange(n, dtype=np.float32) / 8 + 3
    raise KeyError(kind)


# ---------------------------------------------------------------- minmax
MINMAX_N = (1, 2, 1024, 1025, 3000)


def minmax_inputs(n):
    rng = np.random.default_rng(n)
    base = rng.uniform(0.1, 0.6, size=n).astype(np.float32)
    yield "random", base
    yield "constant", np.full(n, 0.375, dtype=np.float32)
    for name, v in (("pos_inf", np.inf), ("neg_inf", -np.inf)):
        x = base.copy()
        x[n // 2] = v
        yield name, x
    if n > 1024:
        x = base.copy()
        x[n - 1] = np.nan
        yield "nan_second_pass", x
    if n > 2050:
        x = base.copy()
        x[2048], x[n - 1] = -4.0, 9.0
        yield "extremes_third_pass", x


# ---------------------------------------------------------------- frame entropy
def entropy_inputs():
    """scores / labels / counts [B, 2, 83]: counts 0, 1, 63, 64, 65 and post, scores of exactly 0
    and 1 inside the counts, and NaN / out-of-range values beyond them."""
    post, ncls = 83, 10
    counts = np.array([[0, 0], [1, 0], [0, 1], [63, 0], [64, 1], [65, 65], [post, post], [0, post],
                       [5, 5], [5, 5], [64, 64]], dtype=np.int32)
    B = counts.shape[0]
    rng = np.random.default_rng(4)
    scores = rng.uniform(0.05, 0.95, size=(B, 2, post)).astype(np.float32)
    labels = rng.integers(0, ncls, size=(B, 2, post)).astype(np.int32)
    scores[8, 0, 2] = 0.0                            # 0 * log(0) = NaN, as in torch
    scores[9, 1, 4] = 1.0
    for b in range(B):
        for t in range(2):
            tail = slice(int(counts[b, t]), post)
            scores[b, t, tail] = np.resize(np.array([np.nan, 2.0, -1.0, np.inf], dtype=np.float32),
                                           post - counts[b, t])
            labels[b, t, tail] = np.resize(np.array([99, -5, ncls], dtype=np.int32), post - counts[b, t])
    cw = rng.uniform(0.5, 2.0, size=ncls).astype(np.float32)
    return scores, labels, counts, cw


# ---------------------------------------------------------------- L1 map
L1_SHAPES = ((130, 7), (70, 512))


def l1_input(n, c):
    rng = np.random.default_rng(n + c)
    f = rng.normal(size=(n, c)).astype(np.float32)
    f[4, :] = np.nan                                 # a frame whose entropy weight was NaN
    f[9, 2] = np.inf
    f[66, 2] = np.inf                                # inf - inf against row 9 gives NaN
    f[66, c - 1] = -np.inf
    return f


# ---------------------------------------------------------------- Euclid map
def euclid_input(n):
    rng = np.random.default_rng(n)
    xy = rng.uniform(-500, 500, size=(n, 2))
    loc = rng.integers(0, 3, size=n).astype(np.int64)
    if n > 10:
        xy[3] = xy[1]                                # coincident points, same and other location
        xy[8] = xy[1]
        loc[1], loc[3], loc[8] = 0, 0, 2
    return xy, loc
