"""GPU suite: every sparse-convolution kernel structure against the float64 reference (spconv_fp64.py).

Error measure (the dense precedent, test_dense_gpu.py::test_conv2d_f16x3_is_fp32_class): per output element
|got - ref| / norm, norm = the reference's abs chain (sum of |a*b| over the products, plus |scale*...|, |shift|,
|residual|); e = its maximum over the layer.  Every structure: e <= 1.5e-6.  The split structures (bf16x6 and f16x3)
also: e <= 3 e_f32 + 1e-8, e_f32 from the f32 MFMA structure on the same input (the VALU one for Cin = 5).

f16 subnormal floor of the f16x3 structures.  The kernels split an activation x into xh = f16(x) and
xl' = f16((x - xh) 2^11) (csrc/sp_rows.h, csrc/glds_common.h).  (x - xh) 2^11 is exact in f32; where it lies below
f16's normal range (|x - xh| < 2^-25, i.e. wherever xh is itself an f16 subnormal, |x| < 2^-14) its rounding to f16
is absolute: half a subnormal ulp, 2^-25, so x is carried to within 2^-25 * 2^-11 = 2^-36.  That is not relative to x
and no fp32 kernel has it, so the split rule gets the per-element absolute term
    2^-36 * |scale| * sum over the gathered taps and channels of |W|.
It is 2^11 below what a kernel that loses the lifted piece would be off by (2^-25 per activation): the xmag = 1e-4
cases still see such a kernel.

Inputs: activations lognormal * normal * xmag (clamped to +-6e4 where f16 structures run), BN scale and shift on the
output's scale (shift ~ 0.1 xmag: a shift of O(1) would hide the convolution at xmag = 1e-4), a residual where
Cin = Cout on submanifold layers."""
import time

import numpy as np
import pytest
import torch

import spconv_fp64 as R
from test_detector_oracle import random_sparse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GEOMS = {"subm": ((3, 3, 3), (1, 1, 1), (0, 0, 0), True),
         "down": ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
         "down011": ((3, 3, 3), (2, 2, 2), (0, 1, 1), False),
         "down311": ((3, 1, 1), (2, 1, 1), (0, 0, 0), False)}
F32 = (False, True)                                  # VALU f32, f32 MFMA
BF16X6 = ("bf16x6", "wave", "wave2")
F16X3 = ("wave2_f16x3", "wave2_f16x3_tiles", "glds_f16x3", "rng_f16x3", "blk_f16x3", "r16_f16x3")
# (128, 16): SpMiddleFHD's first layer behind a 128-channel VFE reader; no matrix-core structure, the VALU kernel alone
PAIRS = [(5, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 16)]


def structures(cin, cout, geom):
    """The structures the library builds for cin -> cout at this geometry (sparse_conv_layer's mfma=)."""
    from al3d.detector_ops import MFMA_PAIRS
    out = [False]
    if (cin, cout) in MFMA_PAIRS:
        out += [True, *BF16X6, "wave2_f16x3", "wave2_f16x3_tiles", "glds_f16x3"]
    if geom == "subm" and (cin, cout) in ((32, 32), (64, 64)):
        out.append("rng_f16x3")
    if geom == "subm" and (cin, cout) in ((32, 32), (64, 64), (128, 128)):
        out.append("blk_f16x3")
    if geom in ("subm", "down") and cin == 16:
        out.append("r16_f16x3")
    return out


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _raster(coords, shape):
    return np.argsort(R.cell_key(coords, shape), kind="stable")


class Case:
    """One layer's inputs (float32, as the device sees them) and their float64 reference."""

    def __init__(self, rng, coords, batch, shape, cin, cout, geom, xmag, relu=True):
        k, s, p, subm = GEOMS[geom]
        n = len(coords)
        self.coords, self.batch, self.shape, self.geom, self.relu = coords, batch, list(shape), geom, relu
        self.k, self.s, self.p, self.subm = k, s, p, subm
        x = rng.normal(size=(n, cin)) * np.exp(rng.normal(size=(n, cin))) * xmag
        if xmag <= 300:
            x = np.clip(x, -6.0e4, 6.0e4)                 # the lognormal tail may not leave f16's range
        self.x = x.astype(np.float32)
        self.w = (rng.normal(size=(*k, cin, cout)) / np.sqrt(cin * np.prod(k))).astype(np.float32)
        self.scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        self.shift = (rng.normal(0, 0.1, cout) * xmag).astype(np.float32)
        self.res = (rng.normal(size=(n, cout)) * xmag).astype(np.float32) if (subm and cin == cout) else None
        self.reference()

    def reference(self, x=None, res=None):
        x = self.x if x is None else x
        res = self.res if res is None else res
        r = R.sparse_conv(x, self.coords, self.shape, self.w, self.k, self.s, self.p, self.subm, self.scale, self.shift,
                          res, relu=self.relu)
        self.ref, self.norm, self.ocoords, self.oshape, self.nbr = r["out"], r["norm"], r["coords"], r["shape"], r["nbr"]
        wa = np.abs(self.w.astype(np.float64)).reshape(self.nbr.shape[1], self.x.shape[1], -1)
        self.floor = 2.0 ** -36 * R.layer(np.ones((len(self.coords), self.x.shape[1])), self.nbr, wa,
                                          np.abs(self.scale.astype(np.float64)))
        return r

    def run(self, mfma, x=None, res=None, io=0, perm=None):
        """The device layer; returns its output rows aligned with the reference's rows (float64, f32 rows)."""
        from al3d import detector_ops as D
        x = self.x if x is None else x
        res = self.res if res is None else res
        coords = self.coords
        if perm is not None:                             # the same layer on permuted input rows
            x, coords = x[perm], coords[perm]
            res = None if res is None else res[perm]
        xt, rt = _t(x), None if res is None else _t(res)
        if io & D.IO_IN_PAIR:
            xt = D.rows_convert(xt, True)
        if rt is not None and io & D.IO_RES_PAIR:
            rt = D.rows_convert(rt, True)
        got, gco, gshape = D.sparse_conv_layer(xt, _t(coords), self.batch, self.shape, _t(self.w), self.k, self.s,
                                               self.p, self.subm, scale=_t(self.scale), shift=_t(self.shift),
                                               residual=rt, relu=self.relu, mfma=mfma, io=io)
        if io & D.IO_OUT_PAIR:
            got = D.rows_convert(got, False)
        got, gco = got.cpu().double().numpy(), gco.cpu().numpy()
        assert gshape == self.oshape, (mfma, gshape, self.oshape)
        # sites: exactly the reference's, as sets (strided rows are in raster order, the reference's in its own)
        kg, kr = R.cell_key(gco, self.oshape), R.cell_key(self.ocoords, self.oshape)
        assert len(kg) == len(kr) and len(np.unique(kg)) == len(kg), mfma
        pos = np.searchsorted(np.sort(kr), kg)
        assert np.array_equal(np.sort(kg), np.sort(kr)), f"{mfma}: output sites differ from the reference's"
        where = np.argsort(kr, kind="stable")[pos]       # reference row of each device row
        out = np.empty_like(got)
        out[where] = got
        return out

    def err(self, got, mask=None):
        d = np.abs(got - self.ref)
        if mask is not None:
            d = d[mask]
            nrm = self.norm[mask]
        else:
            nrm = self.norm
        return float((d / nrm).max()) if d.size else 0.0

    def err_floor(self, got, floor):
        """max (|got - ref| - floor) / norm: e less a derived absolute term (see the header)."""
        d = np.abs(got - self.ref) - floor
        return float((d / self.norm).max()) if d.size else 0.0


def check_structures(case, mfmas, tag=""):
    """Every structure in `mfmas` against the case's reference; the split rule against f32 MFMA (VALU for Cin = 5)."""
    from al3d import detector_ops as D
    errs, split = {}, {}
    for m in mfmas:
        runs = [case.run(m)]
        if m in ("rng_f16x3", "r16_f16x3"):             # raster and random row order (the latter is the case's own)
            saved = D.R16_TPW
            try:
                for tpw in ((0, 1, 3, 64) if m == "r16_f16x3" else (0,)):
                    D.R16_TPW = tpw
                    runs += [case.run(m, perm=_raster(case.coords, case.shape)), case.run(m)]
            finally:
                D.R16_TPW = saved
        assert all(np.isfinite(g).all() for g in runs), m
        errs[m] = max(case.err(g) for g in runs)
        split[m] = max(case.err_floor(g, case.floor if m in F16X3 else 0.0) for g in runs)
    e32 = errs[True if True in errs else False]
    for m, e in errs.items():
        assert e <= 1.5e-6, f"{tag} {m}: e = {e:.3e} > 1.5e-6 (e_f32 = {e32:.3e})"
        if m in BF16X6 or m in F16X3:
            assert split[m] <= 3.0 * e32 + 1e-8, \
                f"{tag} {m}: e = {split[m]:.3e} > 3 e_f32 + 1e-8 (e_f32 = {e32:.3e})"
    return errs


# ---------------------------------------------------------------- 1. every structure, every pair, every geometry
@pytest.mark.parametrize("xmag", [1.0, 1e-4, 300.0, 1e-15, 1e15])
@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_structures_vs_fp64(geom, cin, cout, xmag):
    """f32 and bf16x6 structures claim the whole fp32 range (xmag 1e-15 and 1e15 too); f16x3 ones xmag <= 300."""
    rng = np.random.default_rng(cin * 1000 + cout * 10 + list(GEOMS).index(geom))
    shape, batch, n = [9, 41, 37], 3, 3001
    _, coords = random_sparse(rng, batch, shape, n, 1)
    case = Case(rng, coords, batch, shape, cin, cout, geom, xmag)
    mf = structures(cin, cout, geom)
    if xmag in (1e-15, 1e15):
        mf = [m for m in mf if m in F32 or m in BF16X6]
    errs = check_structures(case, mf, tag=f"{geom} {cin}->{cout} x{xmag:g}")
    print(f"fp64 e {geom} {cin}->{cout} xmag={xmag:g}: " +
          " ".join(f"{m}={e:.2e}" for m, e in errs.items()))


# ---------------------------------------------------------------- 2. edges of the site sets and of the tiling
def _edge_coords(rng, name, shape, batch):
    D_, H_, W_ = shape
    cells = set()

    def rand(b, m):
        while m:
            c = (b, int(rng.integers(D_)), int(rng.integers(H_)), int(rng.integers(W_)))
            if c not in cells:
                cells.add(c)
                m -= 1
    if name == "faces":                                  # voxels on all six faces of the grid
        rand(0, 150)
        rand(2, 150)
        for b in (0, 2):
            for _ in range(15):
                z, y, x = int(rng.integers(D_)), int(rng.integers(H_)), int(rng.integers(W_))
                cells.update({(b, 0, y, x), (b, D_ - 1, y, x), (b, z, 0, x), (b, z, H_ - 1, x), (b, z, y, 0),
                              (b, z, y, W_ - 1)})
    elif name == "single":                               # one voxel in the middle frame
        rand(0, 200)
        cells.add((1, D_ // 2, H_ // 2, W_ // 2))
        rand(2, 200)
    elif name == "empty_frame":                          # an empty frame between two fully occupied ones
        cells.update((b, z, y, x) for b in (0, 2) for z in range(D_) for y in range(H_) for x in range(W_))
    elif name == "block5":                               # 5x5x5 fully occupied: every site inside sees all 27 taps
        cells.update((1, z, y, x) for z in range(1, 6) for y in range(3, 8) for x in range(4, 9))
    elif name.startswith("n"):                           # exact row counts; even cells: a strided row per input
        m = int(name[1:])
        even = [(b, z, y, x) for b in range(batch) for z in range(0, D_, 2) for y in range(0, H_, 2)
                for x in range(0, W_, 2)]
        pick = rng.choice(len(even), m, replace=False)
        cells.update(even[i] for i in pick)
    c = np.array(sorted(cells), dtype=np.int32).reshape(-1, 4)
    rng.shuffle(c)
    return c


EDGE_CASES = ["faces", "single", "empty_frame", "block5"] + [f"n{m}" for m in (31, 32, 33, 127, 128, 129, 255, 256, 257)]
# (geometry, channel pair) runs of each edge case: between them every structure runs at least once
EDGE_RUNS = [("subm", 16, 16), ("subm", 64, 64), ("subm", 128, 128), ("down", 16, 32), ("down011", 32, 64),
             ("down311", 64, 128), ("subm", 128, 16)]


@pytest.mark.parametrize("name", EDGE_CASES)
def test_structures_vs_fp64_edges(name):
    """Odd grid sizes in every dimension (strided layers with odd input sizes), faces, a lone voxel, an empty frame between
    full ones, a fully occupied 5x5x5 block, n = n_out at tile and wave boundaries."""
    rng = np.random.default_rng(len(name) * 7 + sum(map(ord, name)))
    shape, batch = [7, 11, 13], 3
    coords = _edge_coords(rng, name, shape, batch)
    covered = set()
    for geom, cin, cout in EDGE_RUNS:
        for xmag in (1.0, 1e-4):
            case = Case(rng, coords, batch, shape, cin, cout, geom, xmag)
            if name.startswith("n") and geom == "down":
                assert len(case.ocoords) == len(coords)    # even cells: n_out = n
            mf = structures(cin, cout, geom)
            check_structures(case, mf, tag=f"{name} {geom} {cin}->{cout} x{xmag:g}")
            covered.update(mf)
    assert covered == set(F32) | set(BF16X6) | set(F16X3)


@pytest.mark.parametrize("cin,cout", [(16, 32), (128, 128)])
def test_structures_with_no_output_rows(cin, cout):
    """n > 0 inputs, n_out = 0: every input lies past the last window of the padding-free (3,1,1) stride-2 layer."""
    rng = np.random.default_rng(cin)
    shape, batch = [4, 9, 7], 2
    coords = np.array([(b, 3, y, x) for b in range(batch) for y in range(0, 9, 2) for x in range(7)], np.int32)
    case = Case(rng, coords, batch, shape, cin, cout, "down311", 1.0)
    assert len(case.ocoords) == 0
    for m in structures(cin, cout, "down311"):
        got = case.run(m)
        assert got.shape == (0, cout), m


# ---------------------------------------------------------------- 3. pair rows
PAIR_RUNS = [("wave2_f16x3_tiles", "subm", 16, 16), ("wave2_f16x3_tiles", "down", 16, 32),
             ("wave2_f16x3_tiles", "down311", 128, 128), ("glds_f16x3", "subm", 64, 64),
             ("glds_f16x3", "down011", 64, 128), ("rng_f16x3", "subm", 32, 32), ("rng_f16x3", "subm", 64, 64),
             ("blk_f16x3", "subm", 128, 128), ("r16_f16x3", "subm", 16, 16), ("r16_f16x3", "down", 16, 32)]


@pytest.mark.parametrize("xmag", [1.0, 1e-4, 300.0])
@pytest.mark.parametrize("mfma,geom,cin,cout", PAIR_RUNS)
def test_pair_rows_vs_fp64(mfma, geom, cin, cout, xmag):
    """Pair rows (csrc/sp_rows.h; io bits 1 = input, 2 = output, 4 = residual) made by rows_convert from the f32 rows,
    pair outputs read back as xh + xl' 2^-11: against the fp64 result of the ORIGINAL f32 inputs, e <= 1.5e-6.  A stored
    pair row carries 22-23 significant bits, so only this bound applies, not the split rule.  Below f16's normal range a
    stored value is off by up to 2^-36 absolute (the header's floor, now on storage): pair input rows add the same floor
    as the f16x3 kernels' own split (2^-36 |scale| sum |W|), a pair output or a pair residual 2^-36 per element."""
    from al3d import detector_ops as D
    rng = np.random.default_rng(cin + cout + len(mfma) + len(geom))
    shape, batch, n = [9, 41, 37], 3, 3001
    _, coords = random_sparse(rng, batch, shape, n, 1)
    if mfma in ("rng_f16x3", "r16_f16x3"):               # the raster order the encoder feeds these
        coords = coords[_raster(coords, shape)]
    case = Case(rng, coords, batch, shape, cin, cout, geom, xmag)
    ios = [D.IO_IN_PAIR, D.IO_OUT_PAIR, D.IO_IN_PAIR | D.IO_OUT_PAIR]
    if case.res is not None:
        ios += [D.IO_RES_PAIR, D.IO_IN_PAIR | D.IO_OUT_PAIR | D.IO_RES_PAIR]
    for io in ios:
        floor = (case.floor if io & D.IO_IN_PAIR else 0.0) + 2.0 ** -36 * (bool(io & D.IO_OUT_PAIR) + bool(io & D.IO_RES_PAIR))
        e = case.err_floor(case.run(mfma, io=io), floor)
        assert e <= 1.5e-6, f"{mfma} io={io}: e = {e:.3e}"


# ---------------------------------------------------------------- 4. non-finite propagation
NF_RUNS = [(False, "subm", 16, 16), (False, "down", 5, 16), (True, "subm", 32, 32), (True, "down311", 64, 128),
           ("bf16x6", "subm", 32, 32), ("wave", "subm", 64, 64), ("wave2", "subm", 128, 128),
           ("wave2", "down", 16, 32), ("wave2_f16x3", "subm", 32, 32), ("wave2_f16x3", "down011", 32, 64),
           ("wave2_f16x3_tiles", "subm", 16, 16), ("wave2_f16x3_tiles", "down", 32, 64), ("glds_f16x3", "subm", 64, 64),
           ("glds_f16x3", "down011", 64, 128), ("rng_f16x3", "subm", 32, 32), ("rng_f16x3", "subm", 64, 64),
           ("blk_f16x3", "subm", 128, 128), ("r16_f16x3", "subm", 16, 16), ("r16_f16x3", "down", 16, 32)]


@pytest.mark.parametrize("mfma,geom,cin,cout", NF_RUNS)
def test_non_finite_propagation(mfma, geom, cin, cout):
    """The sweep's f16x3 safety net (a finiteness check on the outputs) needs every kernel to carry a non-finite
    gathered value into exactly the outputs that gather it: missing taps and ragged tiles select a zero row (no
    gather-then-mask), ReLU is v <= 0 ? 0 : v (not fmaxf).  One NaN at a time in input row 0, the last row, a row of the
    ragged last tile, a row on a grid face, a residual row; ReLU on and off.  Then 7e4 (beyond f16) in one channel:
    non-finite in exactly the same outputs for the f16x3 structures, finite and within 1.5e-6 for the others."""
    rng = np.random.default_rng(cin * 3 + cout + len(geom))
    shape, batch, n = [9, 41, 37], 3, 1001                # 1001 = 31 tiles of 32 + a ragged tile of 9
    _, coords = random_sparse(rng, batch, shape, n, 1)
    if mfma in ("rng_f16x3", "r16_f16x3"):
        coords = coords[_raster(coords, shape)]
    face = int(np.nonzero((coords[:, 1] == 0) | (coords[:, 2] == shape[1] - 1) | (coords[:, 3] == 0))[0][0])
    rows = {"row 0": 0, "last row": n - 1, "ragged tile": 32 * (n // 32) + 3, "face": face}
    f16 = mfma in F16X3
    for relu in (True, False):
        case = Case(rng, coords, batch, shape, cin, cout, geom, 1.0, relu=relu)
        poisons = [(what, r, None) for what, r in rows.items()]
        if case.res is not None:
            poisons.append(("residual row", n // 2, cin // 2))
        for what, r, rc in poisons:
            x, res = case.x.copy(), None if case.res is None else case.res.copy()
            c = int(rng.integers(cin))
            if what == "residual row":
                res[r, rc] = np.nan
                want = np.zeros(case.ref.shape, bool)
                want[r, rc] = True
            else:
                x[r, c] = np.nan
                want = np.broadcast_to((case.nbr == r).any(1)[:, None], case.ref.shape)
            assert want.any(), what
            got = case.run(mfma, x=x, res=res)
            bad = ~np.isfinite(got)
            assert np.array_equal(bad, want), f"{mfma} relu={relu} NaN in {what}: {int(bad.sum())} non-finite outputs, " \
                                              f"{int(want.sum())} gather it"
            e = case.err(got, ~want)
            assert e <= 1.5e-6, f"{mfma} relu={relu} NaN in {what}: the other outputs moved, e = {e:.3e}"
        # beyond f16's range
        x = case.x.copy()
        r, c = n // 3, int(rng.integers(cin))
        x[r, c] = 7.0e4
        got = case.run(mfma, x=x)
        want = np.broadcast_to((case.nbr == r).any(1)[:, None], case.ref.shape)
        if f16:
            assert np.array_equal(~np.isfinite(got), want), f"{mfma} relu={relu}: 7e4 input"
        else:
            assert np.isfinite(got).all(), f"{mfma} relu={relu}: 7e4 input"
            case.reference(x=x)
            e = case.err(got)
            assert e <= 1.5e-6, f"{mfma} relu={relu} 7e4 input: e = {e:.3e}"


# ---------------------------------------------------------------- 5. the encoder at full size
def test_encoder_full_size_vs_fp64():
    """Two synthetic 10-sweep frames voxelised on the device (60,000-voxel cap hit in both) through the product's own
    rulebook path -- raster level 0, mask sort on levels 2-3, the frame-sorted fast path -- under each arithmetic,
    against encoder_fp64 cell by cell, normalised by the last layer's own abs sum (encoder_fp64 says why not by the
    abs chain through all layers: ~1e27 here).  Bound 1e-5: a first-order sum of 21 layers at <= 3.5e-7 each (the f32
    MFMA figure at K ~ 3,456); f16x3 and bf16x6 within 3x the f32 error."""
    import os
    from al3d import detector_ops as D, synthetic
    from al3d.datasets import DeviceSweepLoader, PoolFrames, generate_task_anchors
    from al3d.models import build_detector
    from al3d.utils import Config
    from test_detector_oracle import G
    cfg = Config.fromfile(os.path.join(os.path.dirname(G), "..", "examples", "active",
                                       "cbgs_spatial_temporal_feature.py"))
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    model = model.to(DEV).eval()
    pool = PoolFrames.from_numpy([synthetic.make_point_cloud(s, nsweeps=10) for s in (4242, 977)], DEV)
    loader = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, batch_size=2, device=DEV)
    ex = next(iter(loader))
    assert ex["num_voxels"].tolist() == [60000, 60000]
    feats, coords = ex["voxel_features"].cpu().numpy(), ex["coordinates"].cpu().numpy()
    sparse_shape = list(np.asarray(ex["shape"][0])[::-1] + [1, 0, 0])
    t0 = time.time()
    ref, norm = R.encoder_fp64(model.backbone, feats, coords, 2, sparse_shape)
    t_ref = time.time() - t0
    saved = D.MATH
    errs = {}
    try:
        for math in ("f16x3", "bf16x6", "f32"):
            D.MATH = math
            with torch.no_grad():
                bev, _ = model.sparse_stage(ex)
            got = bev.cpu().double().numpy()
            assert got.shape == ref.shape, (math, got.shape, ref.shape)
            live = norm > 0
            assert (got[~live] == 0).all(), f"{math}: values at cells without sites"
            errs[math] = float((np.abs(got - ref)[live] / norm[live]).max())
    finally:
        D.MATH = saved
    print(f"encoder fp64 e (reference {t_ref:.1f} s):", {m: f"{e:.3e}" for m, e in errs.items()})
    for math, e in errs.items():
        assert e <= 1e-5, f"{math}: e = {e:.3e}"
    for math in ("f16x3", "bf16x6"):
        assert errs[math] <= 3.0 * errs["f32"], f"{math}: e = {errs[math]:.3e} > 3 e_f32 = {3 * errs['f32']:.3e}"


# ---------------------------------------------------------------- 6. the four-channel VALU layer
@pytest.mark.parametrize("geom", ["subm", "down"])
def test_four_channel_valu_layer_vs_fp64(geom):
    """4 -> 16 (sp_conv_kernel<4, 16>: points without a time channel) is built beside 5 -> 16 and no model of the suite
    selects it: the f32 VALU structure against the float64 reference, e <= 1.5e-6 like every other structure."""
    rng = np.random.default_rng(416 + len(geom))
    shape, batch, n = [9, 41, 37], 3, 3001
    _, coords = random_sparse(rng, batch, shape, n, 1)
    for xmag in (1.0, 1e-15, 1e15):
        case = Case(rng, coords, batch, shape, 4, 16, geom, xmag)
        got = case.run(False)
        assert np.isfinite(got).all()
        e = case.err(got)
        assert e <= 1.5e-6, f"{geom} 4->16 x{xmag:g}: e = {e:.3e}"
