"""CPU suite: the BEV-pooling oracle (oracle/al3d_oracle_detector.c: al3d_oracle_bev_pool) against an independent
torch statement of bevfusion/mmdet3d/models/vtransforms/base.py:127-163 + ops/bev_pool (index_add_ in ascending
point order, then the reference's permute / unbind / cat).  The reference's own op needs its CUDA extension
(bev_pool_ext) and mmcv, both absent: parity unpinned, like spconv and the rotated NMS."""
import numpy as np

import bevpool_cases as cases
from bevpool_cases import torch_bev_pool as _torch_bev_pool          # the torch statement, shared with the GPU regime tests


def test_oracle_bev_pool_equals_torch_statement(oracle):
    rng = np.random.default_rng(0)
    B, P, C = 2, 6000, 7
    nx, dx, bx = [12, 9, 3], [0.5, 0.75, 2.0], [-2.75, -3.0, -2.0]
    geom = np.stack([rng.uniform(-4.0, 4.0, P), rng.uniform(-4.5, 4.5, P), rng.uniform(-4, 4, P)], 1).astype(np.float32)
    geom[5] = np.nan
    geom[7, 0] = -3.2                       # t in (-1, 0): .long() truncates to cell 0 -- kept by the reference
    x = rng.normal(size=(P, C)).astype(np.float32)
    ref = _torch_bev_pool(x, geom, B, dx, bx, nx).numpy()                   # [B, Dz*C, H, W]
    lo = np.asarray(bx, np.float32) - np.asarray(dx, np.float32) / np.float32(2)
    got = oracle.bev_pool(x, geom, B, lo, dx, nx)                           # [B, H, W, Dz*C]
    assert got.shape == (B, 12, 9, 3 * C)
    assert np.array_equal(got.transpose(0, 3, 1, 2).view(np.int32), ref.view(np.int32))
    assert np.abs(got).sum() > 0


def test_oracle_bev_pool_fused_outer_product_equals_materialised(oracle):
    rng = np.random.default_rng(1)
    B, N, D, fH, fW, C = 2, 3, 5, 4, 6, 8
    depth = rng.uniform(0, 1, (B * N, D, fH, fW)).astype(np.float32)
    ctx = rng.normal(size=(B * N, fH, fW, C)).astype(np.float32)
    x = (depth[..., None] * ctx[:, None]).astype(np.float32)                # depth_lss.py:93: materialised [BN,D,fH,fW,C]
    geom = rng.uniform(-3, 3, (B * N * D * fH * fW, 3)).astype(np.float32)
    lo, dx, nx = [-2, -2, -3], [0.4, 0.4, 6.0], [10, 10, 1]
    a = oracle.bev_pool(x.reshape(-1, C), geom, B, lo, dx, nx)
    b = oracle.bev_pool(ctx.reshape(-1, C), geom, B, lo, dx, nx, depth=depth.reshape(-1), D=D, fHW=fH * fW)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.abs(a).sum() > 0


def test_regime_case_builder_holds_every_list_regime_and_the_oracle_equals_torch(oracle):
    """The input of tests/test_bevpool_regimes_gpu.py.  Precondition first: recounted with the reference's
    ((geom - lo) / dx).long(), the named cells hold exactly 0 / 1 / 127 / 128 | 129 / 8192 | 8193 / 9000 members (the three
    list regimes of csrc/bev_pool.hip and both boundaries), on consecutive cell ids, so the GPU test cannot silently lose a
    regime; the fused-form input likewise.  Then the oracle equals the torch statement on it, bit for bit."""
    geom = cases.regimes_geom()
    n = cases.assert_counts(geom, cases.REGIME_COUNTS)
    assert geom.shape[0] % cases.B == 0 and 70000 < geom.shape[0] < 82000
    named = set(cases.REGIME_COUNTS[0])
    rest = np.array([n[0, c] for c in range(n.shape[1]) if c not in named])
    assert rest.min() == 0 and rest.max() == 24                                  # the background everywhere else
    assert n[1].max() == 1000 and (n[1] > 256).sum() == 4 and n.sum() < geom.shape[0]     # and padding outside the grid
    assert not np.array_equal(np.argsort(geom[:, 0], kind="stable"), np.arange(len(geom)))
    lss = cases.lss_geom()
    Bs, N, D, fH, fW = cases.LSS_SHAPE
    assert lss.shape[0] == Bs * N * D * fH * fW
    cases.assert_counts(lss, cases.LSS_COUNTS)
    lo = cases.grid_lo()
    rng = np.random.default_rng(2)
    for C in (80, 6):
        x = rng.normal(size=(geom.shape[0], C)).astype(np.float32)
        ref = _torch_bev_pool(x, geom, cases.B, cases.DX, cases.BX, cases.NX).numpy()
        got = oracle.bev_pool(x, geom, cases.B, lo, cases.DX, cases.NX)
        assert np.array_equal(cases.as_reference_layout(got).view(np.int32), ref.view(np.int32))


def test_boundary_case_oracle_equals_torch_statement(oracle):
    """Hand-placed points at every edge of the cell rule (t = 0, (-1, 0), -1, nx - 2^-k, nx, NaN, inf, 1e30; first and last
    cell; first and last index of a sample): the reference's expression keeps exactly the expected number, and the oracle
    equals the torch statement."""
    geom, kept = cases.boundary_geom()
    n = cases.cell_counts(geom, cases.B)
    assert n.sum() == kept and n[0, 0] >= 1 and n[1, 0] >= 1 and n[0, -1] >= 1 and n[1, -1] >= 1
    assert np.array_equal(n[0], n[1])
    x = np.random.default_rng(3).normal(size=(geom.shape[0], 5)).astype(np.float32)
    ref = _torch_bev_pool(x, geom, cases.B, cases.DX, cases.BX, cases.NX).numpy()
    got = oracle.bev_pool(x, geom, cases.B, cases.grid_lo(), cases.DX, cases.NX)
    assert np.array_equal(cases.as_reference_layout(got).view(np.int32), ref.view(np.int32))
