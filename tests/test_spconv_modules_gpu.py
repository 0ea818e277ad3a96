"""GPU suite of al3d.spconv: every layer type against the float64 yardsticks of spconv_mod_fp64.py.

Error measure and bound are test_spconv_fp64_gpu.py's (imported, not restated): e = max |got - ref| / norm <= 1.5e-6 with
norm the reference's abs chain; under f16x3 less that file's derived 2^-36 floor term.  An unfused f32 step (an unfolded
BatchNorm) adds 2^-24 on the same normaliser.  A chain of layers is held to the sum of its steps' bounds, element by
element (each step's own bound plus what it carries of the steps before).  Max pool and dense() are exact.

Shapes: B = 2, spatial_shape (5, 12, 11), about 300 active sites: odd sizes in every dimension, ten 32-row tiles with a
ragged last one, two 256-row pitches."""
import numpy as np
import pytest
import torch

import spconv_fp64 as R
import spconv_mod_fp64 as M
from test_detector_oracle import random_sparse, to_dense
from test_spconv_fp64_gpu import DEV, GEOMS, Case, _t

pytestmark = pytest.mark.gpu
B, SHAPE, N = 2, [5, 12, 11], 300
BOUND = 1.5e-6
STEP = 2.0 ** -24
MATHS = ["f16x3", "bf16x6", "f32"]


class use_math:
    """D.MATH switched the way the fp64 suite does it."""

    def __init__(self, math):
        self.math = math

    def __enter__(self):
        from al3d import detector_ops as D
        self.saved, D.MATH = D.MATH, self.math

    def __exit__(self, *exc):
        from al3d import detector_ops as D
        D.MATH = self.saved


def _sites(seed, n=N, batch=B):
    rng = np.random.default_rng(seed)
    return rng, random_sparse(rng, batch, SHAPE, n, 1)[1]


def _load(mod, w, bias=None):
    with torch.no_grad():
        mod.weight.copy_(torch.from_numpy(np.asarray(w)))
        if bias is not None:
            mod.bias.copy_(torch.from_numpy(np.asarray(bias)))
    return mod.to(DEV).eval()


def _tensor(x, coords, shape=SHAPE, batch=B):
    import al3d.spconv as spconv
    return spconv.SparseConvTensor(_t(np.asarray(x, np.float32)), _t(np.asarray(coords, np.int32)), list(shape), batch)


def _measure(ref, math):
    """A test_spconv_fp64_gpu.Case holding only a reference: its err / err_floor are the suite's error measure."""
    c = object.__new__(Case)
    c.ref, c.norm = ref["out"], ref["norm"]
    floor = ref["floor"] if math == "f16x3" else 0.0
    return lambda got: c.err_floor(np.asarray(got, np.float64), floor)


def _rows(t):
    return t.features.cpu().double().numpy(), t.indices.cpu().numpy()


def _raster_sorted(coords, shape):
    key = R.cell_key(coords, shape)
    return bool((np.diff(key) > 0).all())


# ---------------------------------------------------------------- convolutions
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("cin,cout", [(16, 32), (5, 7)])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_conv_layers_vs_fp64(geom, cin, cout, bias, math):
    import al3d.spconv as spconv
    rng, coords = _sites(11 + list(GEOMS).index(geom) + cin)
    case = Case(rng, coords, B, SHAPE, cin, cout, geom, 1.0, relu=False)
    case.scale = np.ones(cout, np.float32)
    case.shift = (rng.normal(0, 0.1, cout) if bias else np.zeros(cout)).astype(np.float32)
    case.res = None
    case.reference()
    k, s, p, subm = GEOMS[geom]
    mod = spconv.SubMConv3d(cin, cout, k, bias=bias) if subm else spconv.SparseConv3d(cin, cout, k, s, p, bias=bias)
    _load(mod, case.w, case.shift if bias else None)
    with use_math(math):
        out = mod(_tensor(case.x, coords))
    got, gco = _rows(out)
    assert list(out.spatial_shape) == case.oshape
    assert np.array_equal(gco, case.ocoords), "site set / row order differs from the yardstick's"
    if not subm:
        assert _raster_sorted(gco, case.oshape)
    e = case.err_floor(got, case.floor if math == "f16x3" else 0.0)
    print(f"e {geom} {cin}->{cout} bias={bias} {math}: {e:.3e}")
    assert np.isfinite(got).all() and e <= BOUND, f"e = {e:.3e}"


@pytest.mark.parametrize("cin,cout", [(16, 32), (5, 7)])
def test_kernel_size_one_is_a_gemm_on_the_input_sites(cin, cout):
    """spconv's quirk: kernel size 1 returns the input's indices and shape whatever the stride."""
    import al3d.spconv as spconv
    rng, coords = _sites(5)
    x = rng.normal(size=(len(coords), cin)).astype(np.float32)
    w = (rng.normal(size=(1, 1, 1, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = rng.normal(0, 0.1, cout).astype(np.float32)
    mod = _load(spconv.SparseConv3d(cin, cout, 1, stride=2), w, b)
    xt = _tensor(x, coords)
    out = mod(xt)
    got, gco = _rows(out)
    assert out.indices is xt.indices and list(out.spatial_shape) == SHAPE and np.array_equal(gco, coords)
    w2 = w.reshape(cin, cout).astype(np.float64)
    ref = dict(out=x.astype(np.float64) @ w2 + b, norm=np.abs(x.astype(np.float64)) @ np.abs(w2) + np.abs(b),
               floor=M.F16_FLOOR * np.ones((len(x), cin)) @ np.abs(w2))
    e = _measure(ref, "f16x3")(got)
    assert e <= BOUND, f"e = {e:.3e}"


# ---------------------------------------------------------------- row counts
def _conv_pair(rng, coords, batch=B):
    """One submanifold and one strided 16 -> 32 layer on `coords` against the yardstick; returns the two outputs."""
    import al3d.spconv as spconv
    outs = []
    for geom in ("subm", "down"):
        k, s, p, subm = GEOMS[geom]
        x = rng.normal(size=(len(coords), 16)).astype(np.float32)
        w = (rng.normal(size=(*k, 16, 32)) / np.sqrt(16 * 27)).astype(np.float32)
        b = rng.normal(0, 0.1, 32).astype(np.float32)
        mod = _load(spconv.SubMConv3d(16, 32, k) if subm else spconv.SparseConv3d(16, 32, k, s, p), w, b)
        out = mod(_tensor(x, coords, batch=batch))
        ref = M.conv(x, coords, SHAPE, w, k, s, p, subm, bias=b)
        got, gco = _rows(out)
        assert got.shape == ref["out"].shape and np.array_equal(gco, ref["coords"]) and list(out.spatial_shape) == ref["shape"]
        e = _measure(ref, "f16x3")(got)
        assert e <= BOUND, f"{geom} n={len(coords)}: e = {e:.3e}"
        outs.append(out)
    return outs


@pytest.mark.parametrize("n", [31, 32, 33, 255, 256, 257])
def test_row_counts_at_tile_and_pitch_boundaries(n):
    rng, coords = _sites(n, n=n)
    assert len(coords) == n
    _conv_pair(rng, coords)


def test_no_rows():
    import al3d.spconv as spconv
    rng = np.random.default_rng(0)
    coords = np.zeros((0, 4), np.int32)
    for out in _conv_pair(rng, coords):
        assert tuple(out.features.shape) == (0, 32) and tuple(out.indices.shape) == (0, 4)
    x = _tensor(np.zeros((0, 16), np.float32), coords)
    pooled = spconv.SparseMaxPool3d(3, 2, 1)(x)
    assert tuple(pooled.features.shape) == (0, 16) and list(pooled.spatial_shape) == [3, 6, 6]
    up = _load(spconv.SparseConvTranspose3d(16, 32, 2, 2), np.zeros((2, 2, 2, 16, 32), np.float32))(x)
    assert tuple(up.features.shape) == (0, 32) and list(up.spatial_shape) == [10, 24, 22]
    assert float(x.dense().abs().sum()) == 0.0 and tuple(x.dense().shape) == (B, 16, *SHAPE)


def test_one_empty_frame():
    rng, coords = _sites(77)
    coords = coords.copy()
    coords[:, 0] = 1                                           # frame 0 of the two holds nothing
    coords = np.unique(coords, axis=0).astype(np.int32)
    rng.shuffle(coords)
    for out in _conv_pair(rng, coords):
        assert (out.indices[:, 0] == 1).all()


# ---------------------------------------------------------------- inverse conv
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("cin,cmid,cout", [(16, 32, 32), (5, 7, 5)])
@pytest.mark.parametrize("k,s,p", [((2, 2, 2), (2, 2, 2), (0, 0, 0)), ((3, 3, 3), (2, 2, 2), (1, 1, 1))], ids=["k2s2", "k3s2p1"])
def test_inverse_conv_vs_fp64(k, s, p, cin, cmid, cout, math):
    """Paired through indice_key with a strided layer; the matrix-core pair reads the tiled inverse table, the VALU pair
    the plain one.  The yardstick takes the device's forward output as its input: the inverse step alone."""
    import al3d.spconv as spconv
    rng, coords = _sites(31 + cin + k[0])
    x = rng.normal(size=(len(coords), cin)).astype(np.float32)
    wf = (rng.normal(size=(*k, cin, cmid)) / np.sqrt(cin * np.prod(k))).astype(np.float32)
    wi = (rng.normal(size=(*k, cmid, cout)) / np.sqrt(cmid * np.prod(k))).astype(np.float32)
    bi = rng.normal(0, 0.1, cout).astype(np.float32)
    fwd = _load(spconv.SparseConv3d(cin, cmid, k, s, p, bias=False, indice_key="pair"), wf)
    inv = _load(spconv.SparseInverseConv3d(cmid, cout, k, indice_key="pair"), wi, bi)
    with use_math(math):
        xt = _tensor(x, coords)
        mid = fwd(xt)
        out = inv(mid)
    assert out.indices.data_ptr() == xt.indices.data_ptr() and torch.equal(out.indices, xt.indices)
    assert list(out.spatial_shape) == SHAPE
    xm, cm = _rows(mid)
    ref = M.inverse_conv(xm, cm, B, mid.spatial_shape, wi, s, p, coords, SHAPE, bias=bi)
    got, _ = _rows(out)
    e = _measure(ref, math)(got)
    print(f"e inverse {k} {cmid}->{cout} {math}: {e:.3e}")
    assert np.isfinite(got).all() and e <= BOUND, f"e = {e:.3e}"


def test_inverse_conv_needs_its_pair():
    import al3d.spconv as spconv
    from al3d.lib import Al3dError
    rng, coords = _sites(3)
    x = _tensor(rng.normal(size=(len(coords), 16)), coords)
    with pytest.raises(Al3dError, match="indice_key"):
        spconv.SparseInverseConv3d(16, 16, 3, indice_key="nobody").to(DEV)(x)
    mid = spconv.SparseConv3d(16, 16, 3, 2, 1, indice_key="d").to(DEV)(x)
    with pytest.raises(Al3dError, match="kernel_size"):
        spconv.SparseInverseConv3d(16, 16, 2, indice_key="d").to(DEV)(mid)


# ---------------------------------------------------------------- transposed conv
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("cin,cout", [(16, 32), (5, 7)])
@pytest.mark.parametrize("k,s,p,op", [((2, 2, 2), (2, 2, 2), (0, 0, 0), (0, 0, 0)), ((3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1))],
                         ids=["k2s2", "k3s2p1op1"])
def test_transposed_conv_vs_fp64(k, s, p, op, cin, cout, math):
    import al3d.spconv as spconv
    rng, coords = _sites(57 + cin + k[0])
    x = rng.normal(size=(len(coords), cin)).astype(np.float32)
    w = (rng.normal(size=(*k, cin, cout)) / np.sqrt(cin * np.prod(k))).astype(np.float32)
    b = rng.normal(0, 0.1, cout).astype(np.float32)
    if any(op):       # the 3-D class has no output_padding argument in spconv 1.x: the base class carries it
        mod = spconv.SparseConvolution(3, cin, cout, k, s, p, transposed=True, output_padding=op)
    else:
        mod = spconv.SparseConvTranspose3d(cin, cout, k, s, p)
    _load(mod, w, b)
    with use_math(math):
        out = mod(_tensor(x, coords))
    ref = M.transposed_conv(x, coords, B, SHAPE, w, s, p, op, bias=b)
    got, gco = _rows(out)
    assert list(out.spatial_shape) == ref["shape"] == [(SHAPE[d] - 1) * s[d] - 2 * p[d] + k[d] + op[d] for d in range(3)]
    assert np.array_equal(gco, ref["coords"]), "site set / raster order differs from the yardstick's"
    e = _measure(ref, math)(got)
    print(f"e transposed {k} {cin}->{cout} {math}: {e:.3e}")
    assert np.isfinite(got).all() and e <= BOUND, f"e = {e:.3e}"


# ---------------------------------------------------------------- max pool
@pytest.mark.parametrize("C", [1, 5, 64])
@pytest.mark.parametrize("k,s,p", [((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((2, 2, 2), (2, 2, 2), (0, 0, 0))], ids=["k3s2p1", "k2s2"])
def test_max_pool_is_exact(k, s, p, C):
    import al3d.spconv as spconv
    rng, coords = _sites(91 + C)
    x = rng.normal(size=(len(coords), C)).astype(np.float32)
    neg = -np.abs(x) - 1.0
    nan = x.copy()
    nan[rng.random(x.shape) < 0.2] = np.nan
    nan[0] = np.nan                                            # a whole row, and (zero_floor=False) windows of only NaN
    for name, v in (("random", x), ("negative", neg), ("nan", nan)):
        for zero_floor in (True, False):
            out = spconv.SparseMaxPool3d(k, s, p, zero_floor=zero_floor)(_tensor(v, coords))
            ref = M.max_pool(v, coords, SHAPE, k, s, p, zero_floor=zero_floor)
            got, gco = _rows(out)
            assert np.array_equal(gco, ref["coords"]) and list(out.spatial_shape) == ref["shape"]
            assert np.array_equal(got, ref["out"]), f"{name} zero_floor={zero_floor}"
            assert not np.isnan(got).any()
            if name == "negative":
                assert (got == 0).all() if zero_floor else (got < 0).all()
            if name == "random" and not zero_floor:            # the true maximum, stated without the helper
                first = ref["nbr"][0][ref["nbr"][0] >= 0]
                assert np.array_equal(got[0], v[first].max(0).astype(np.float64))


# ---------------------------------------------------------------- indice_key
class _Calls:
    def __init__(self, monkeypatch):
        from al3d import lib
        self.names = []
        real = lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        monkeypatch.setattr(lib, "call", call)

    def count(self, word):
        return sum(word in n for n in self.names)


def test_one_key_builds_one_table(monkeypatch):
    import al3d.spconv as spconv
    from al3d.lib import Al3dError
    rng, coords = _sites(13)
    x = _tensor(rng.normal(size=(len(coords), 16)), coords)
    a, b = spconv.SubMConv3d(16, 16, 3, indice_key="s").to(DEV), spconv.SubMConv3d(16, 16, 3, indice_key="s").to(DEV)
    d1, d2 = spconv.SparseConv3d(16, 16, 3, 2, 1, indice_key="d").to(DEV), spconv.SparseConv3d(16, 16, 3, 2, 1, indice_key="d").to(DEV)
    calls = _Calls(monkeypatch)
    y = b(a(x))
    assert calls.count("_table") == 1 and calls.count("al3d_sp_subm_table") == 1
    entry = y.find_indice_pair("s")
    assert len(entry) == 5 and entry[0] is x.indices and entry[1] is x.indices and entry[3] == SHAPE
    o1 = d1(y)
    o2 = d2(y)
    assert calls.count("_table") == 2 and calls.count("al3d_sp_down_sites") == 1
    assert o1.indices is o2.indices
    with pytest.raises(Al3dError, match="indice_key"):
        spconv.SparseConv3d(16, 16, 3, 1, 1, indice_key="d").to(DEV)(y)          # another stride
    with pytest.raises(Al3dError, match="indice_key"):
        spconv.SparseConv3d(16, 16, 3, 2, 0, indice_key="d").to(DEV)(y)          # another padding
    with pytest.raises(Al3dError, match="indice_key"):
        spconv.SubMConv3d(16, 16, (3, 1, 1), indice_key="s").to(DEV)(y)          # another kernel
    assert calls.count("_table") == 2


def test_inverse_output_keeps_its_pairs_index_grid(monkeypatch):
    """The U-Net pattern: a submanifold layer after the inverse one looks up the grid of the pair's input sites, which exists."""
    import al3d.spconv as spconv
    rng, coords = _sites(29)
    x = _tensor(rng.normal(size=(len(coords), 16)), coords)
    pre = spconv.SubMConv3d(16, 16, 3, indice_key="a").to(DEV)
    down = spconv.SparseConv3d(16, 16, 3, 2, 1, indice_key="d").to(DEV)
    up = spconv.SparseInverseConv3d(16, 16, 3, indice_key="d").to(DEV)
    post = spconv.SubMConv3d(16, 16, 3, indice_key="b").to(DEV)
    calls = _Calls(monkeypatch)
    y = up(down(pre(x)))
    assert calls.count("al3d_sp_scatter_index") == 1
    z = post(y)
    assert calls.count("al3d_sp_scatter_index") == 1 and calls.count("al3d_sp_subm_table") == 2
    assert z.indices is x.indices


# ---------------------------------------------------------------- BatchNorm folding
def _bn(rng, c):
    bn = torch.nn.BatchNorm1d(c, eps=1e-3)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, c)))
        bn.bias.copy_(torch.from_numpy(rng.normal(0, 0.1, c)))
        bn.running_mean.copy_(torch.from_numpy(rng.normal(0, 0.1, c)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, c)))
    return bn


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("geom", ["subm", "down"])
def test_bn_relu_fold_is_one_launch_with_the_layer_bits(geom, math, monkeypatch):
    import al3d.spconv as spconv
    from al3d import detector_ops as D
    rng, coords = _sites(23)
    k, s, p, subm = GEOMS[geom]
    x = rng.normal(size=(len(coords), 16)).astype(np.float32)
    w = (rng.normal(size=(*k, 16, 32)) / np.sqrt(16 * 27)).astype(np.float32)
    b = rng.normal(0, 0.1, 32).astype(np.float32)
    conv = spconv.SubMConv3d(16, 32, k) if subm else spconv.SparseConv3d(16, 32, k, s, p)
    net = spconv.SparseSequential(_load(conv, w, b), _bn(rng, 32), torch.nn.ReLU()).to(DEV).eval()
    scale, shift = D.fold_bn(net[1])
    shift = shift + net[0].bias.detach().float() * scale
    sc64 = scale.cpu().double().numpy()
    ref = R.sparse_conv(x, coords, SHAPE, w, k, s, p, subm, sc64, shift.cpu().double().numpy(), relu=True)
    ref["floor"] = M.conv(x, coords, SHAPE, w, k, s, p, subm)["floor"] * np.abs(sc64)
    with use_math(math):
        want, wco, _ = D.sparse_conv_layer(_t(x), _t(coords), B, SHAPE, _t(w), k, s, p, subm, scale=scale, shift=shift,
                                           relu=True)
        calls = _Calls(monkeypatch)
        out = net(_tensor(x, coords))
        assert calls.count("al3d_sp_conv") == 1
        assert torch.equal(out.features, want) and torch.equal(out.indices, wco), "folded launch differs from sparse_conv_layer"
        e = _measure(ref, math)(_rows(out)[0])
        assert e <= BOUND, f"folded: e = {e:.3e}"
        monkeypatch.setattr(spconv, "FOLD_BN", False)
        plain = net(_tensor(x, coords))
        e = _measure(ref, math)(_rows(plain)[0])
        print(f"e unfolded {geom} {math}: {e:.3e}")
        assert e <= BOUND + STEP, f"unfolded: e = {e:.3e}"


# ---------------------------------------------------------------- dense()
def test_dense_equals_a_scatter_of_the_rows():
    rng, coords = _sites(41)
    x = rng.normal(size=(len(coords), 5)).astype(np.float32)
    t = _tensor(x, coords)
    want = to_dense(x, coords, B, SHAPE)
    assert np.array_equal(t.dense().cpu().numpy(), want)
    assert np.array_equal(t.dense(channels_first=False).cpu().numpy(), want.transpose(0, 2, 3, 4, 1))


# ---------------------------------------------------------------- a small U-shaped net
@pytest.mark.parametrize("math", MATHS)
def test_u_shaped_net_vs_fp64_chain(math):
    """submanifold -> strided (key d1) -> submanifold -> inverse (key d1) -> max pool -> ToDense, a ReLU after each conv.

    The summed bound of its steps, element by element: every conv step may add 1.5e-6 of its own abs sum (under f16x3 plus
    its 2^-36 floor term), and what the steps before it left is carried through its |W| (first order); ReLU and max are
    1-Lipschitz, the pool takes the largest budget of its taps, the scatter is exact.  Not one normaliser through all
    layers: the abs chain grows by sum |W| per layer while the values do not, so after four layers any bound relative
    to it holds for a kernel that is wrong in the fourth digit (spconv_fp64.encoder_fp64 says the same)."""
    import al3d.spconv as spconv
    rng, coords = _sites(67)
    x = rng.normal(size=(len(coords), 16)).astype(np.float32)
    specs = [(16, 16), (16, 32), (32, 32), (32, 32)]
    ws = [(rng.normal(size=(3, 3, 3, ci, co)) / np.sqrt(ci * 27)).astype(np.float32) for ci, co in specs]
    bs = [rng.normal(0, 0.1, co).astype(np.float32) for _, co in specs]
    net = spconv.SparseSequential(
        _load(spconv.SubMConv3d(16, 16, 3, indice_key="s0"), ws[0], bs[0]), torch.nn.ReLU(),
        _load(spconv.SparseConv3d(16, 32, 3, 2, padding=1, indice_key="d1"), ws[1], bs[1]), torch.nn.ReLU(),
        _load(spconv.SubMConv3d(32, 32, 3, indice_key="s1"), ws[2], bs[2]), torch.nn.ReLU(),
        _load(spconv.SparseInverseConv3d(32, 32, 3, indice_key="d1"), ws[3], bs[3]), torch.nn.ReLU(),
        spconv.SparseMaxPool3d(2, 2), spconv.ToDense()).to(DEV).eval()
    with use_math(math):
        got = net(_tensor(x, coords)).cpu().double().numpy()
    one, two, k3 = (1, 1, 1), (2, 2, 2), (3, 3, 3)

    def step(r):
        """ReLU, and the budget so far: this step's own bound + what it carried."""
        own = BOUND * r["norm"] + ((r["floor"] - r["carried"]) if math == "f16x3" else 0.0)
        return dict(r, out=np.maximum(r["out"], 0.0), budget=own + r["carried"])
    r = step(M.conv(x, coords, SHAPE, ws[0], k3, one, one, True, bias=bs[0]))
    r = step(M.conv(r["out"], coords, SHAPE, ws[1], k3, two, one, False, bias=bs[1], xfloor=r["budget"]))
    mc, ms = r["coords"], r["shape"]
    r = step(M.conv(r["out"], mc, ms, ws[2], k3, one, one, True, bias=bs[2], xfloor=r["budget"]))
    r = step(M.inverse_conv(r["out"], mc, B, ms, ws[3], two, one, coords, SHAPE, bias=bs[3], xfloor=r["budget"]))
    r = M.max_pool(r["out"], coords, SHAPE, two, two, (0, 0, 0), xfloor=r["budget"])
    c = r["coords"]
    ref, budget = np.zeros((2, B, 32, *r["shape"]))
    ref[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = r["out"]
    budget[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = r["carried"]
    assert got.shape == ref.shape == (B, 32, 2, 6, 5)
    live = budget > 0
    assert live.any() and (got[~live] == 0).all()
    ratio = float((np.abs(got - ref)[live] / budget[live]).max())
    print(f"e u-net {math}: {ratio:.3f} of the summed bound")
    assert ratio <= 1.0, f"|got - ref| reaches {ratio:.3f} of the summed bound"


# ---------------------------------------------------------------- coordinate check
@pytest.mark.parametrize("row,bit", [((0, SHAPE[0], 3, 3), 2), ((-1, 1, 3, 3), 1)], ids=["z=D", "batch=-1"])
def test_bad_coordinates_are_refused_before_any_grid_kernel(row, bit, monkeypatch):
    """al3d_sp_coords_check reads only the coordinate array: it is called here on its own, with no grid in existence."""
    import al3d.spconv as spconv
    from al3d import lib
    from al3d.lib import Al3dError
    rng, coords = _sites(19)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    good = _t(coords)
    lib.call("al3d_sp_coords_check", good.data_ptr(), len(coords), B, *SHAPE, status.data_ptr(),
             torch.cuda.current_stream().cuda_stream)
    assert int(status.item()) == 0
    coords = coords.copy()
    coords[len(coords) // 2] = row
    bad = _t(coords)
    lib.call("al3d_sp_coords_check", bad.data_ptr(), len(coords), B, *SHAPE, status.data_ptr(),
             torch.cuda.current_stream().cuda_stream)
    assert int(status.item()) == bit
    x = _tensor(rng.normal(size=(len(coords), 16)), coords)
    calls = _Calls(monkeypatch)
    for mod in (spconv.SubMConv3d(16, 16, 3).to(DEV), spconv.SparseConv3d(16, 16, 3, 2, 1).to(DEV),
                spconv.SparseConvTranspose3d(16, 16, 2, 2).to(DEV), spconv.SparseMaxPool3d(2, 2), spconv.ToDense()):
        with pytest.raises(Al3dError, match="indices outside"):
            mod(x)
    assert set(calls.names) == {"al3d_sp_coords_check"}, calls.names
