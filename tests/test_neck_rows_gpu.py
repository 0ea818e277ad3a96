"""GPU suite: the dense neck's first 3x3 fed from the sparse encoder's rows (``detector_ops.BevRows``: the rows input of
``conv3x3_f16x3_frag_kernel`` + ``al3d_sp_bev_index``) against the dense hand-over it replaces -- ``dense_nhwc`` followed by
the same ``conv2d_nhwc``.  The rows input stages the values the dense map holds and only leaves out MFMAs whose A operand
is all +0, so the comparison is on the int32 view of the output: equal word for word, no tolerance."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, COUT = 2, 128
SIZES = [(8, 64), (10, 40)]          # 2 x 2 full 4 x 32 tiles; ragged tiles in both directions
CHANNELS = [32, 128]                 # per row; the map has 2 * C channels


def _occupancy(case, H, W):
    """[B, H, W, 2] bool: which (pixel, z) hold a row."""
    rng = np.random.default_rng(sum(map(ord, case)) + 131 * H + W)
    occ = np.zeros((B, H, W, 2), dtype=bool)
    if case == "full":
        occ[:] = True
    elif case == "frame_empty":
        occ[0] = rng.random((H, W, 1)) < 0.5
    elif case.startswith("pixel_"):
        y, x = {"pixel_3_31": (3, 31), "pixel_4_32": (4, 32), "pixel_0_0": (0, 0), "pixel_last": (H - 1, W - 1)}[case]
        occ[:, y, x, :] = True
    elif case in ("z0_only", "z1_only"):
        occ[..., int(case[1])] = rng.random((B, H, W)) < 0.3
    elif case == "random20":
        pix = rng.random((B, H, W)) < 0.2
        both = rng.random((B, H, W)) < 0.9
        z = rng.integers(0, 2, (B, H, W))
        occ[..., 0] = pix & (both | (z == 0))
        occ[..., 1] = pix & (both | (z == 1))
    elif case == "one_row":
        occ[:, 4, :, :] = True       # first image row of the second tile row: the last halo row of the tiles above
    else:
        raise KeyError(case)
    return occ


CASES = ["full", "frame_empty", "pixel_3_31", "pixel_4_32", "pixel_0_0", "pixel_last", "z0_only", "z1_only", "random20",
         "one_row"]


def _level(occ, C, seed):
    """rows [n, C] f32 and coords [n, 4] i32 (b, z, y, x) of the occupied sites, in a shuffled (non-raster) order."""
    b, y, x, z = np.nonzero(occ)
    order = np.random.default_rng(seed).permutation(len(b))
    coords = np.stack([b, z, y, x], axis=1)[order].astype(np.int32).reshape(-1, 4)
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(len(b), C, generator=g)
    rows[rows.abs() < 0.05] = 0.0                                   # exact zeros inside present rows too
    return rows.to(DEV), torch.from_numpy(coords).to(DEV)


@functools.lru_cache(maxsize=None)
def _layer(C):
    """The frag3x3 weights of a 2C -> 128 layer, a BN scale and a shift of both signs (ReLU(shift) pixels of both kinds)."""
    from al3d import detector_ops as D
    g = torch.Generator().manual_seed(7 + C)
    w = torch.randn(COUT, 2 * C, 3, 3, generator=g) / (18 * C) ** 0.5
    scale = torch.rand(COUT, generator=g) + 0.5
    shift = torch.randn(COUT, generator=g) * 0.3
    wp, sc = D.dense_pack("frag3x3", D.pack_conv_weight(w).to(DEV), scale.to(DEV))
    return wp, sc, shift.to(DEV)


def _both(case, H, W, C, **kw):
    """(rows-input output, dense-input output) of the same layer; ``kw`` goes to both conv2d_nhwc calls."""
    from al3d import detector_ops as D
    from al3d.models.backbones import FPNSpMiddleResNetFHD, SparseTensor
    occ = _occupancy(case, H, W)
    rows, coords = _level(occ, C, seed=H * W + C)
    wp, sc, shift = _layer(C)
    dense = FPNSpMiddleResNetFHD.dense_nhwc(SparseTensor(rows, coords, [2, H, W], B))
    assert int((dense != 0).any(dim=-1).sum()) <= int(occ.any(axis=-1).sum())
    outs = []
    for x in (D.BevRows(rows, coords, D.bev_index(coords, rows.shape[0], B, (2, H, W))), dense):
        k = dict(kw)
        if "out" in k:
            k["out"] = torch.full_like(k["out"], -7.0)
        outs.append(D.conv2d_nhwc(x, wp, sc, shift, 3, 1, 1, True, **k))
    torch.cuda.synchronize()
    return outs


def _same_words(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("H,W", SIZES)
def test_rows_input_equals_dense_input(H, W, C, case):
    got, ref = _both(case, H, W, C)
    assert got.shape == ref.shape == (B, H, W, COUT)
    assert bool(torch.isfinite(ref).all())
    assert _same_words(got, ref)
    if case == "frame_empty":        # ReLU(shift) everywhere, the long way and the short way
        _, _, shift = _layer(C)
        assert _same_words(got[1], torch.relu(shift).expand(H, W, COUT))


@pytest.mark.parametrize("H,W", SIZES)
def test_rows_input_pair_pixel_output(H, W):
    from al3d import detector_ops as D
    got, ref = _both("random20", H, W, 32, io=D.IO_OUT_PAIR)
    assert _same_words(got, ref)


@pytest.mark.parametrize("H,W", SIZES)
def test_rows_input_into_a_channel_window(H, W):
    """A window the 16-byte stores cannot serve (coff = 2): the untransposed f32 epilogue, neighbours untouched."""
    out = torch.empty((B, H, W, COUT + 6), dtype=torch.float32, device=DEV)
    got, ref = _both("random20", H, W, 32, out=out, coff=2)
    assert _same_words(got, ref)
    assert bool((got[..., :2] == -7.0).all()) and bool((got[..., COUT + 2:] == -7.0).all())


def test_rows_input_is_refused_where_it_is_not_built(monkeypatch):
    from al3d import detector_ops as D, lib
    H, W, C = 8, 64, 32
    rows, coords = _level(_occupancy("random20", H, W), C, seed=1)
    wp, sc, shift = _layer(C)
    x = D.BevRows(rows, coords, D.bev_index(coords, rows.shape[0], B, (2, H, W)))
    monkeypatch.setattr(D, "NECK_IN", "dense")
    with pytest.raises(lib.Al3dError):
        D.conv2d_nhwc(x, wp, sc, shift, 3, 1, 1, True)


@pytest.mark.parametrize("n_case", ["some", "none"])
def test_bev_index_matches_numpy_scatter(n_case):
    from al3d import detector_ops as D
    H, W = 10, 40
    occ = _occupancy("random20", H, W) if n_case == "some" else np.zeros((B, H, W, 2), dtype=bool)
    _, coords = _level(occ, 8, seed=3)
    n = coords.shape[0]
    assert (n == 0) == (n_case == "none")
    got = D.bev_index(coords, n, B, (2, H, W)).cpu().numpy()
    ref = np.full((B, H, W, 2), -1, dtype=np.int32)
    c = coords.cpu().numpy()
    ref[c[:, 0], c[:, 2], c[:, 3], c[:, 1]] = np.arange(n, dtype=np.int32)
    assert got.dtype == np.int32 and np.array_equal(got, ref)


def test_bev_index_is_built_for_two_levels_only():
    from al3d import detector_ops as D, lib
    coords = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(lib.Al3dError):
        D.bev_index(coords, 1, 1, (3, 8, 8))
