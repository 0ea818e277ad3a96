"""CPU suite: the yardstick of tests/test_spatial_edges_gpu.py.

The GPU file compares the kNN and shortest-path kernels with the C oracle bit for bit.  Here the
oracle itself is pinned on the same inputs (tests/spatial_cases.py): its kNN to a numpy brute force
with a stable sort, its Dijkstra to scipy's, and the inputs to the properties they are there for.
Non-finite poses have no outside yardstick (cKDTree raises on them): for those two families only
the graph side is compared, and that both frames end up without an edge."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra

import spatial_cases as S


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _brute_knn(xy, kq):
    n = xy.shape[0]
    dx = xy[None, :, 0] - xy[:, None, 0]
    dy = xy[None, :, 1] - xy[:, None, 1]
    d2 = dx * dx
    d2 = d2 + dy * dy                                 # two roundings, never one fused
    idx = np.argsort(d2, axis=1, kind="stable")[:, :kq]
    d = np.sqrt(np.take_along_axis(d2, idx, axis=1))
    if n < kq:                                        # scipy pads missing neighbours with (inf, n)
        d = np.concatenate([d, np.full((n, kq - n), np.inf)], axis=1)
        idx = np.concatenate([idx, np.full((n, kq - n), n)], axis=1)
    return d, idx.astype(np.int64)


def _graph(oracle, label):
    if label in S.TABLE_LABELS:
        _, (kd, ki), _, rows = S.table_case(label)
    else:
        _, xy, kq, rows = S.point_case(label)
        kd, ki = oracle.knn(xy, kq)
    return kd.shape[0], rows, oracle.knn_csr(kd, ki)


def _oracle_rows(oracle, csr, rows):
    if len(rows) == csr[0].shape[0] - 1:
        return oracle.apsp(*csr)
    return np.stack([oracle.apsp(*csr, int(r), int(r) + 1)[0] for r in rows])


def test_lds_split_is_where_the_cap_is():
    n = S.last_lds_n()
    assert S.sssp_lds_bytes(n) <= S.LDS_CAP < S.sssp_lds_bytes(n + 1)
    assert n < 2 ** 15 < S.MAX_N                      # the largest chain needs the 16th id bit


@pytest.mark.parametrize("label", [l for l in S.FINITE_POINT_LABELS if l != "clusters"])
def test_oracle_knn_is_the_stable_brute_force(oracle, label):
    _, xy, kq, _ = S.point_case(label)
    assert xy.shape[0] <= S.ALL_ROWS_MAX_N
    d0, i0 = _brute_knn(xy, kq)
    d1, i1 = oracle.knn(xy, kq)
    assert np.array_equal(i0, i1)
    assert np.array_equal(_bits(d0), _bits(d1))


@pytest.mark.parametrize("label", S.POINT_LABELS + S.TABLE_LABELS)
def test_oracle_apsp_is_scipy_dijkstra(oracle, label):
    n, rows, (indptr, indices, weights) = _graph(oracle, label)
    ref = dijkstra(csr_matrix((weights, indices, indptr), shape=(n, n)), directed=True, indices=rows)
    got = _oracle_rows(oracle, (indptr, indices, weights), rows)
    assert np.array_equal(_bits(ref), _bits(got))


# ---------------------------------------------------------------- the inputs are what they claim
def test_stopped_has_long_runs_and_isolated_frames(oracle):
    assert S.stopped_longest_run() > S.STOPPED_KQ
    n, _, csr = _graph(oracle, "stopped")
    D = oracle.apsp(*csr)
    alone = np.isinf(D).sum(axis=1) == n - 1
    assert alone.any() and not alone.all()
    assert np.array_equal(alone, np.diff(csr[0]) == 0)


@pytest.mark.parametrize("label", ["clusters", "clusters_lds"])
def test_clusters_are_mostly_unreachable(oracle, label):
    _, rows, csr = _graph(oracle, label)
    share = np.isinf(_oracle_rows(oracle, csr, rows)).mean()
    assert 0.5 < share < 0.999


@pytest.mark.parametrize("label", S.STAR_LABELS)
def test_star_hub_has_every_edge(oracle, label):
    n, _, csr = _graph(oracle, label)
    assert np.diff(csr[0]).max() == n - 1 > 16


@pytest.mark.parametrize("label", S.CHAIN_LABELS)
def test_chain_row_is_the_running_sum(oracle, label):
    n, rows, csr = _graph(oracle, label)
    assert 0 in rows and n - 1 in rows
    row = oracle.apsp(*csr, 0, 1)[0]
    total = 0.0
    for w in S.chain_weights(n).tolist():             # plain left-to-right f64 sum
        total += w
    assert np.isfinite(row).all() and row[n - 1] == total


def test_chain_sizes_sit_on_both_sides_of_the_split():
    sizes = sorted(S.table_case(l)[1][0].shape[0] for l in S.CHAIN_LABELS)
    assert sizes == [S.last_lds_n(), S.last_lds_n() + 1, S.MAX_N]
    assert S.table_case("chain_of_stars")[1][0].shape[0] > S.last_lds_n()
    assert S.point_case("clusters")[1].shape[0] > S.last_lds_n() >= S.point_case("clusters_lds")[1].shape[0]


@pytest.mark.parametrize("label", S.NONFINITE_LABELS)
def test_nonfinite_frames_get_no_edge(oracle, label):
    _, xy, _, _ = S.point_case(label)
    bad = np.nonzero(~np.isfinite(xy).all(axis=1))[0]
    assert len(bad) == 2 and np.isnan(xy[bad[0]]).any() and np.isinf(xy[bad[1]]).any()
    n, _, csr = _graph(oracle, label)
    deg = np.diff(csr[0])
    assert (deg[bad] == 0).all() and (np.delete(deg, bad) > 0).all()
    D = oracle.apsp(*csr)
    assert (np.isinf(D[bad]).sum(axis=1) == n - 1).all() and (D[bad, bad] == 0).all()
