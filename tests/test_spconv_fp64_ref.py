"""CPU suite: the float64 sparse-convolution reference (spconv_fp64.py) against dense float64 ``F.conv3d``.

The GPU suite (test_spconv_fp64_gpu.py) holds every sparse kernel structure to this reference, so the reference is
checked here on its own: at the four geometries of FPNSpMiddleResNetFHD, on odd grid sizes, batch 3 with an empty
middle frame, output values, normaliser and (strided layers) the site set against max-pooled occupancy."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spconv_fp64 as R

GEOMS = [(True, (3, 3, 3), (1, 1, 1), (0, 0, 0)),
         (False, (3, 3, 3), (2, 2, 2), (1, 1, 1)),
         (False, (3, 3, 3), (2, 2, 2), (0, 1, 1)),
         (False, (3, 1, 1), (2, 1, 1), (0, 0, 0))]


def _sparse(rng, batch, shape, n, c, empty=()):
    frames = [b for b in range(batch) if b not in empty]
    cells = set()
    while len(cells) < n:
        cells.add((int(rng.choice(frames)), int(rng.integers(shape[0])), int(rng.integers(shape[1])),
                   int(rng.integers(shape[2]))))
    coords = np.array(sorted(cells), dtype=np.int32)
    rng.shuffle(coords)
    return rng.normal(size=(len(coords), c)), coords


def _dense(feats, coords, batch, shape):
    d = np.zeros((batch, feats.shape[1], *shape), dtype=np.float64)
    d[coords[:, 0], :, coords[:, 1], coords[:, 2], coords[:, 3]] = feats
    return torch.from_numpy(d)


def _conv3d(x, w, k, s, p, subm):
    wt = torch.from_numpy(np.ascontiguousarray(np.transpose(w, (4, 3, 0, 1, 2))))
    pad = [q // 2 for q in k] if subm else list(p)
    return F.conv3d(x, wt, stride=(1, 1, 1) if subm else s, padding=pad)


@pytest.mark.parametrize("subm,k,s,p", GEOMS)
@pytest.mark.parametrize("shape", [[7, 9, 11], [5, 13, 3]])
def test_reference_layer_equals_dense_conv3d(subm, k, s, p, shape):
    rng = np.random.default_rng(sum(shape) + sum(k) * 3 + sum(p))
    batch, cin, cout = 3, 4, 6
    n = int(0.3 * 2 * np.prod(shape))
    feats, coords = _sparse(rng, batch, shape, n, cin, empty=(1,))
    w = rng.normal(size=(*k, cin, cout))
    scale, shift = rng.uniform(0.5, 1.5, cout), rng.normal(size=cout)
    res = rng.normal(size=(n, cout)) if subm else None
    got = R.sparse_conv(feats, coords, shape, w, k, s, p, subm, scale, shift, res, relu=True)
    oc, oshape = got["coords"], got["shape"]
    assert oshape == (shape if subm else R.out_shape(shape, k, s, p))
    # sites
    occ = _dense(np.ones((n, 1)), coords, batch, shape)
    if subm:
        assert np.array_equal(oc, coords)
    else:
        pooled = F.max_pool3d(occ, k, s, p)[:, 0] > 0
        assert list(pooled.shape[1:]) == oshape
        want = np.argwhere(pooled.numpy()).astype(np.int32)             # (b, z, y, x), ascending
        assert np.array_equal(oc, want)
        assert not (oc[:, 0] == 1).any()                                 # nothing comes out of the empty frame
    # values and normaliser, sampled at the sites
    y = _conv3d(_dense(feats, coords, batch, shape), w, k, s, p, subm).numpy()
    ya = _conv3d(_dense(np.abs(feats), coords, batch, shape), np.abs(w), k, s, p, subm).numpy()
    at = (oc[:, 0], slice(None), oc[:, 1], oc[:, 2], oc[:, 3])
    ref = y[at] * scale + shift
    nref = ya[at] * scale + np.abs(shift)
    if res is not None:
        ref, nref = ref + res, nref + np.abs(res)
    np.testing.assert_allclose(got["out"], np.maximum(ref, 0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["norm"], nref, rtol=1e-12, atol=1e-12)
    # the table: every live tap names an input row of the right frame
    nbr = got["nbr"]
    live = nbr >= 0
    assert (coords[nbr[live], 0] == np.broadcast_to(oc[:, :1], nbr.shape)[live]).all()
    if subm:
        assert (nbr[:, nbr.shape[1] // 2] == np.arange(n)).all()        # the centre tap is the site itself


def test_reference_relu_keeps_nan_and_empty_inputs():
    nbr = np.array([[0, -1], [-1, -1], [1, 0]])
    x = np.array([[np.nan], [-1.0]])
    w = np.ones((2, 1, 2))
    out = R.layer(x, nbr, w, relu=True)
    assert np.isnan(out[0]).all() and (out[1] == 0).all() and np.isnan(out[2]).all()
    oc, osh = R.strided_sites(np.zeros((0, 4), np.int32), [5, 5, 5], (3, 3, 3), (2, 2, 2), (1, 1, 1))
    assert oc.shape == (0, 4) and osh == [3, 3, 3]
    # an input past the last window of a padding-free layer claims no output
    oc, osh = R.strided_sites(np.array([[0, 3, 0, 0]], np.int32), [4, 1, 1], (3, 1, 1), (2, 1, 1), (0, 0, 0))
    assert oc.shape == (0, 4) and osh == [1, 1, 1]


def test_encoder_reference_equals_dense_emulation():
    """encoder_fp64 over the whole FPNSpMiddleResNetFHD against a dense float64 emulation (conv3d + max-pooled site
    masks, BN/ReLU on active sites), on a small grid whose every level keeps some sites."""
    from al3d import synthetic
    from al3d.models.backbones import FPNSpMiddleResNetFHD
    rng = np.random.default_rng(8)
    shape, batch = [41, 16, 16], 2
    feats, coords = _sparse(rng, batch, shape, 700, 5)
    enc = FPNSpMiddleResNetFHD(num_input_features=5)
    synthetic.seeded_init_(enc, seed=5)
    enc.eval()
    bev, norm = R.encoder_fp64(enc, feats, coords, batch, shape)

    x = _dense(feats, coords, batch, shape)
    mask = _dense(np.ones((len(coords), 1)), coords, batch, shape)

    def conv(m, x):
        w = m.weight.detach().double().numpy()
        y = _conv3d(x, w, m.kernel_size, m.stride, m.padding, m.subm)
        return y if m.bias is None else y + m.bias.detach().double().view(1, -1, 1, 1, 1)

    def bn(m, y):
        sh = (1, -1, 1, 1, 1)
        return (y - m.running_mean.double().view(sh)) / torch.sqrt(m.running_var.double().view(sh) + m.eps) \
            * m.weight.detach().double().view(sh) + m.bias.detach().double().view(sh)

    for seq in enc._stages():
        mods = list(seq.children())
        i = 0
        while i < len(mods):
            m = mods[i]
            name = type(m).__name__
            if name in ("SubMConv3d", "SparseConv3d"):
                if not m.subm:
                    mask = (F.max_pool3d(mask, m.kernel_size, m.stride, m.padding) > 0).double()
                x = torch.relu(bn(mods[i + 1], conv(m, x))) * mask
                i += 3
            elif name == "SparseBasicBlock":
                y = torch.relu(bn(m.bn1, conv(m.conv1, x))) * mask
                x = torch.relu(bn(m.bn2, conv(m.conv2, y)) * mask + x) * mask
                i += 1
            else:
                i += 1
    B, C, D_, H_, W_ = x.shape
    ref = x.reshape(B, C * D_, H_, W_).permute(0, 2, 3, 1).numpy()
    assert bev.shape == ref.shape == (batch, 2, 2, 256)
    assert mask.sum() > 0 and np.abs(ref).max() > 0
    np.testing.assert_allclose(bev, ref, rtol=1e-10, atol=1e-12 * np.abs(ref).max())
    assert (norm >= np.abs(bev) * (1 - 1e-12)).all() and ((norm > 0) == (mask.permute(0, 3, 4, 1, 2)
                                                                           .reshape(B, H_, W_, D_).repeat(1, 1, 1, C) > 0)
                                                          .numpy()).all()
