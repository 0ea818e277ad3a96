"""GPU suite: the spatial term's kernels (csrc/apsp_kernels.hip: exact 2-D kNN, the symmetric
kNN-graph adjacency, one label-correcting shortest-path sweep per source) against the C oracle,
bit for bit, on the inputs of tests/spatial_cases.py: exact distance ties, stopped vehicles,
components, hubs, n - 1 rounds, both label paths at the size where one hands over to the other,
16-bit node ids, kq and tile limits, non-finite poses.  tests/test_spatial_cases_cpu.py pins the
oracle on the same inputs to numpy and scipy.  There is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import spatial_cases as S

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


def _same_bits(got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float64
    assert np.array_equal(np.isinf(got), np.isinf(ref))
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))


_GRAPHS = {}


def _graph(oracle, label):
    """(knn_d, knn_i, oracle CSR, rows) of a family, the kNN table from the oracle; made once."""
    if label not in _GRAPHS:
        if label in S.TABLE_LABELS:
            _, (kd, ki), _, rows = S.table_case(label)
        else:
            _, xy, kq, rows = S.point_case(label)
            kd, ki = oracle.knn(xy, kq)
        _GRAPHS[label] = kd, ki, oracle.knn_csr(kd, ki), rows
    return _GRAPHS[label]


# ---------------------------------------------------------------- kNN
@pytest.mark.parametrize("label", S.POINT_LABELS)
def test_knn_edges(hip, oracle, label):
    _, xy, kq, _ = S.point_case(label)
    d0, i0 = _graph(oracle, label)[:2]
    d1, i1 = hip.knn(xy, kq)
    assert np.array_equal(i0, i1)
    nan = np.isnan(d0)
    assert np.array_equal(nan, np.isnan(d1))
    assert nan.any() == (label in S.NONFINITE_LABELS)
    assert np.array_equal(d0.view(np.int64)[~nan], d1.view(np.int64)[~nan])


# ---------------------------------------------------------------- shortest paths
@pytest.mark.parametrize("label", S.POINT_LABELS + S.TABLE_LABELS)
def test_geodesic_edges(hip, ops, oracle, label):
    kd, ki, csr, rows = _graph(oracle, label)
    n = kd.shape[0]
    if n <= S.ALL_ROWS_MAX_N:
        assert len(rows) == n
        ref = oracle.apsp(*csr)
        kd_t, ki_t = _d(kd), _d(ki)                  # one upload for the n + 1 calls
        _same_bits(ops.apsp_knn(kd_t, ki_t).cpu().numpy(), ref)
        got = torch.cat([ops.apsp_knn(kd_t, ki_t, int(r), 1) for r in rows]).cpu().numpy()
    else:
        ref = np.stack([oracle.apsp(*csr, int(r), int(r) + 1)[0] for r in rows])
        got = np.stack([hip.apsp_rows(kd, ki, int(r), 1)[0] for r in rows])
    _same_bits(got, ref)
    assert (got[np.arange(len(rows)), rows] == 0).all()
    alone = np.diff(csr[0])[rows] == 0               # a frame without an edge: inf off the diagonal
    assert (np.isinf(got[alone]).sum(axis=1) == n - 1).all()
    if label == "stopped":
        assert alone.any()
    if label in S.NONFINITE_LABELS:
        bad = ~np.isfinite(S.point_case(label)[1]).all(axis=1)
        assert bad.sum() == 2 and alone[bad].all()


@pytest.mark.parametrize("label", ["uniform-n700", "chain_of_stars"])
def test_row_blocks_equal_rows_of_the_full_map(hip, ops, oracle, label):
    kd, ki = _graph(oracle, label)[:2]
    n = kd.shape[0]
    assert (n > S.last_lds_n()) == (label == "chain_of_stars")
    kd_t, ki_t = _d(kd), _d(ki)
    full = ops.apsp_knn(kd_t, ki_t).view(torch.int64)          # stays on the device
    for m in (1, 5):
        for r0 in (0, 1, n - m):
            block = ops.apsp_knn(kd_t, ki_t, r0, m)
            assert block.shape == (m, n)
            assert torch.equal(block.view(torch.int64), full[r0:r0 + m]), (r0, m)
    assert torch.equal(_d(hip.apsp_rows(kd, ki, n - 5, 5)).view(torch.int64), full[n - 5:])
    for r0 in (0, 3, n):
        empty = ops.apsp_knn(kd_t, ki_t, r0, 0)
        assert empty.shape == (0, n) and empty.dtype == torch.float64


# ---------------------------------------------------------------- refusals
def test_limits_are_refused():
    """Every refusal comes before the first launch: the tensors are far smaller than the sizes named."""
    from al3d import lib
    n = 8
    xy = torch.zeros(n, 2, dtype=torch.float64, device=DEV)
    kd = torch.zeros(n, 33, dtype=torch.float64, device=DEV)
    ki = torch.zeros(n, 33, dtype=torch.int64, device=DEV)
    out = torch.zeros(n, n, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def apsp(n_, kq, row0, nrows):
        lib.call("al3d_apsp_knn_rows_f64", kd.data_ptr(), ki.data_ptr(), n_, kq, row0, nrows, out.data_ptr(),
                 ws.data_ptr(), stream)

    def knn(kq):
        lib.call("al3d_knn_2d_f64", xy.data_ptr(), n, kq, kd.data_ptr(), ki.data_ptr(), stream)

    with pytest.raises(lib.Al3dError, match="n must be < 65536"):
        apsp(65536, 2, 0, 1)
    for kq in (33, 0):
        with pytest.raises(lib.Al3dError, match=r"al3d_apsp_knn_f64: kq must be in \[1,32\]"):
            apsp(n, kq, 0, 1)
        with pytest.raises(lib.Al3dError, match=r"al3d_knn_2d_f64: kq must be in \[1,32\]"):
            knn(kq)
    for row0, nrows in ((n - 1, 2), (n, 1), (0, n + 1), (-1, 1)):
        with pytest.raises(lib.Al3dError, match="bad row range"):
            apsp(n, 2, row0, nrows)
    torch.cuda.synchronize()
    assert not out.any() and not kd.any() and not ki.any()      # nothing was written
