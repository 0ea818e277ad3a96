"""Inputs for the BEV-pooling tests (CPU: tests/test_bevpool_oracle.py, GPU: tests/test_bevpool_regimes_gpu.py) and the
torch statement of the reference both compare with.

csrc/bev_pool.hip orders a cell's member list one of three ways -- rank counting in the wave (len <= 128), a bitonic
sort in LDS (128 < len <= 8192), rank counting by a workgroup (len > 8192) -- and bev_sum_vec_kernel serves one to four
cells per wave, walking long lists in 128-entry chunks while short cells idle.  ``build_geom`` places EXACT member counts
on chosen cell ids, so a test can put every regime, both boundaries and a mixed wave into one small input and assert
(``cell_counts``) that it did."""
import functools

import numpy as np
import torch

NX = (24, 20, 2)
DX = (0.5, 0.5, 4.0)
BX = (-5.75, -4.75, -2.0)
B = 2
FAR = 1.0e3                                   # padding points: far outside every grid of these tests

# consecutive cell ids of sample 0.  Cells per wave of bev_sum_vec_kernel: 1 (C = 256), 2 (C = 128), 3 (C = 80), 4 (C <= 64):
#   4 per wave: {0..3} = rank-fallback / short / empty / short-at-the-boundary, {4..7} = sorted / short / sorted-at-the-cap / 1,
#               {8..11} = background / rank-fallback-just-over-the-cap / sorted / short
#   3 per wave: {0,1,2} = 9000 / 100 / 0, {3,4,5} = 128 / 129 / 127, {6,7,8}, {9,10,11} = 8193 / 300 / 64
#   2 per wave: {0,1} = 9000 / 100, {2,3} = 0 / 128, {4,5} = 129 / 127, {6,7} = 8192 / 1
REGIME_COUNTS = ({0: 9000, 1: 100, 2: 0, 3: 128, 4: 129, 5: 127, 6: 8192, 7: 1, 9: 8193, 10: 300, 11: 64, 12: 65},
                 {37: 257, 38: 1000, 500: 600, 959: 513})          # sample 1: a few sorted lists; 959 = the last cell
# the same for the fused form at B = 2, N = 2, D = 12, fH x fW = 16 x 48: 18,432 points per sample
LSS_SHAPE = (2, 2, 12, 16, 48)                # B, N, D, fH, fW
LSS_COUNTS = ({0: 8193, 1: 100, 2: 0, 3: 128, 4: 129, 5: 127, 6: 8192, 7: 1, 9: 300, 10: 64, 11: 65},
              {37: 257, 38: 1000, 500: 600, 959: 513})


def grid_lo(dx=DX, bx=BX):
    """(bx - dx / 2) in float32, as the reference computes it."""
    return np.asarray(bx, np.float32) - np.asarray(dx, np.float32) / np.float32(2)


def build_geom(counts, background, seed, nx=NX, dx=DX, bx=BX, per_sample=None):
    """counts: per sample a map {cell id -> member count}, cell id = (ix * nx1 + iy) * nx2 + iz inside the sample; every
    cell a map does not name gets a count drawn from background = (lo, hi), inclusive.  Each point sits at its cell's
    origin plus a jitter in [0.1, 0.9] of the cell size; each sample is padded to the same length (``per_sample``, or the
    longest sample) with points far outside the grid and then shuffled, so arrival order differs from point order.
    -> geom [len(counts) * per_sample, 3] float32."""
    rng = np.random.default_rng(seed)
    nx = np.asarray(nx, np.int64)
    dx64, lo64 = np.asarray(dx, np.float64), grid_lo(dx, bx).astype(np.float64)
    ncell = int(nx.prod())
    samples = []
    for named in counts:
        n = rng.integers(background[0], background[1] + 1, ncell)
        for cid, k in named.items():
            n[cid] = k
        cid = np.repeat(np.arange(ncell), n)
        idx = np.stack([cid // (nx[1] * nx[2]), (cid // nx[2]) % nx[1], cid % nx[2]], 1)
        g = lo64 + (idx + rng.uniform(0.1, 0.9, idx.shape)) * dx64
        samples.append(g.astype(np.float32))
    per = max(len(g) for g in samples) if per_sample is None else per_sample
    assert all(len(g) <= per for g in samples), [len(g) for g in samples]
    out = np.full((len(samples), per, 3), FAR, np.float32)
    for b, g in enumerate(samples):
        out[b, :len(g)] = g
        rng.shuffle(out[b], axis=0)
    return out.reshape(-1, 3)


def cell_counts(geom, nsample, nx=NX, dx=DX, bx=BX):
    """Members per cell with the reference's expression ((geom - (bx - dx / 2)) / dx).long() (base.py:136,147-154)
    -> int64 [nsample, nx0 * nx1 * nx2]."""
    dxt, bxt = torch.tensor(dx, dtype=torch.float32), torch.tensor(bx, dtype=torch.float32)
    g = ((torch.from_numpy(geom) - (bxt - dxt / 2.0)) / dxt).long()
    nxt = torch.tensor(nx)
    kept = ((g >= 0) & (g < nxt)).all(1)
    per = geom.shape[0] // nsample
    b = torch.arange(geom.shape[0]) // per
    ncell = int(nxt.prod())
    lin = (b * ncell + (g[:, 0] * nx[1] + g[:, 1]) * nx[2] + g[:, 2])[kept]
    return torch.bincount(lin, minlength=nsample * ncell).view(nsample, ncell).numpy()


def assert_counts(geom, counts, nx=NX, dx=DX, bx=BX):
    """The precondition of the regime tests: every named cell holds exactly its count."""
    got = cell_counts(geom, len(counts), nx, dx, bx)
    for b, named in enumerate(counts):
        for cid, k in named.items():
            assert got[b, cid] == k, (b, cid, int(got[b, cid]), k)
    return got


@functools.lru_cache(maxsize=None)
def regimes_geom():
    """Every list regime, both boundaries and mixed waves in one input (about 76 k points, 960 cells per sample).
    Built once and shared: callers do not write to it."""
    g = build_geom(REGIME_COUNTS, (0, 24), seed=41)
    return g


@functools.lru_cache(maxsize=None)
def lss_geom():
    """The same regimes inside the point count of the fused form's (B, N, D, fH, fW) = LSS_SHAPE."""
    _, N, D, fH, fW = LSS_SHAPE
    g = build_geom(LSS_COUNTS, (0, 1), seed=42, per_sample=N * D * fH * fW)
    return g


def boundary_geom(nx=NX, dx=DX, bx=BX, nsample=B):
    """Hand-placed points at the edges of ``bev_axis_cell``, per axis with the other two coordinates mid-cell:
    t = (g - lo) / dx exactly 0; t in (-1, 0) (truncation keeps these as cell 0); t exactly -1; t = nx - 2^-k;
    t exactly nx; NaN, +-inf, +-1e30; plus the first and the last cell of each sample, and a kept point at the last
    index of sample 0 and at the first index of sample 1 (every sample holds the same cells: a point counted to the
    wrong sample changes two cells' sums).
    -> geom [P, 3] float32 with P % nsample == 0, and the number of points the reference keeps."""
    lo = grid_lo(dx, bx).astype(np.float64)
    dx64, nx64 = np.asarray(dx, np.float64), np.asarray(nx, np.float64)
    mid = lo + (np.floor(nx64 / 2) + 0.5) * dx64
    rows, kept = [], 0
    for k in range(3):
        ts = [(0.0, 1), (-0.5, 1), (-2.0 ** -20, 1), (-1.0 + 2.0 ** -10, 1), (-1.0, 0), (-1.0 - 2.0 ** -10, 0),
              (nx64[k] - 0.5, 1), (nx64[k] - 2.0 ** -10, 1), (nx64[k] - 2.0 ** -18, 1), (nx64[k], 0), (nx64[k] + 0.5, 0),
              (1.0, 1), (nx64[k] - 1.0, 1)]                     # and two interior cell edges
        for t, keep in ts:
            g = mid.copy()
            g[k] = lo[k] + t * dx64[k]
            rows.append(g)
            kept += keep
        for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            g = mid.copy()
            g[k] = bad
            rows.append(g)
    first, last = lo + 0.5 * dx64, lo + (nx64 - 0.5) * dx64
    body = np.asarray(rows, np.float32)
    per = len(body) + 4
    out = np.empty((nsample, per, 3), np.float32)
    for b in range(nsample):
        # [first cell | the hand-placed rows | last cell, mid cell, mid cell]: index 0 and index per - 1 of every sample are kept
        out[b] = np.concatenate([first[None], body, last[None], mid[None], mid[None]]).astype(np.float32)
        out[b, 1:-1] = np.roll(out[b, 1:-1], 7 * b, axis=0)
    return out.reshape(-1, 3), nsample * (kept + 4)


def torch_bev_pool(x, geom, B, dx, bx, nx):
    """The reference expressions (base.py:127-163 + ops/bev_pool), with index_add_ -- which adds in ascending row order on
    the CPU -- standing in for sort + segmented sum.  -> [B, Dz*C, H, W] torch float32."""
    Np = x.shape[0]
    x, geom = torch.from_numpy(x), torch.from_numpy(geom)
    dx, bx = torch.tensor(dx, dtype=torch.float32), torch.tensor(bx, dtype=torch.float32)
    g = ((geom - (bx - dx / 2.0)) / dx).long()
    batch_ix = torch.cat([torch.full([Np // B, 1], ix, dtype=torch.long) for ix in range(B)])
    g = torch.cat((g, batch_ix), 1)
    kept = (g[:, 0] >= 0) & (g[:, 0] < nx[0]) & (g[:, 1] >= 0) & (g[:, 1] < nx[1]) & (g[:, 2] >= 0) & (g[:, 2] < nx[2])
    x, g = x[kept], g[kept]
    H, W, Dz, C = nx[0], nx[1], nx[2], x.shape[1]
    out = torch.zeros(B * Dz * H * W, C)
    lin = ((g[:, 3] * Dz + g[:, 2]) * H + g[:, 0]) * W + g[:, 1]           # out[b, z, x, y, c] (bev_pool_cuda.cu:33-36)
    out.index_add_(0, lin, x)
    out = out.view(B, Dz, H, W, C).permute(0, 4, 1, 2, 3).contiguous()     # bev_pool.py:96
    return torch.cat(out.unbind(dim=2), 1)                                  # base.py:161 -> [B, Dz*C, H, W]


def as_reference_layout(out):
    """This build's [B, nx0, nx1, nz*C] -> the reference's [B, nz*C, nx0, nx1] (same channel order iz*C + c)."""
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))
