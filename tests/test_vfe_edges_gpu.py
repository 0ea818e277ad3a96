"""GPU suite: the fused VFE reader (csrc/vfe.hip) at its sizes, counts, LDS launch shapes, padded-slot rules, NaN rule and
refusals, on the cases of tests/vfe_cases.py (whose own conditions tests/test_vfe_cases_cpu.py checks).

Accuracy, per case: e = max |got - ref64| / absum (tests/vfe_fp64.py).  Two gates:
  - e <= B, the first-order worst case of the f32 chains (vfe_fp64.bound), as in tests/test_vfe_gpu.py;
  - e <= 3 e32 + 1e-8, e32 the largest error of three float32 evaluations of the same formula on the same case
    (vfe_fp64.e32: ascending k, descending k, numpy's float32 matmul; computed on the host, never from the kernel).  The
    factor and the floor are the split rule of tests/test_spconv_fp64_gpu.py.  B is 60 to 5,000 times looser than that.
M <= 300 everywhere."""
import ctypes

import numpy as np
import pytest
import torch

import vfe_cases as C
import vfe_fp64 as V

pytestmark = pytest.mark.gpu
ENTRY, ENTRY_LAUNCH = "al3d_vfe_net_f32", "al3d_vfe_net_launch_f32"


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _net(c, use_norm=None):
    from al3d.models import build_reader
    if use_norm is None:
        use_norm = "norm.weight" in c["params"]
    mod = build_reader(dict(type="VoxelFeatureExtractorV2", num_input_features=c["F"], use_norm=use_norm,
                            num_filters=list(c["filters"]), with_distance=c["wd"]))
    sd = mod.state_dict()
    sd.update({k: torch.from_numpy(np.asarray(v)) for k, v in c["params"].items()})
    mod.load_state_dict(sd, strict=True)
    return mod.cuda().eval().net(torch.device("cuda"))


def _gates(tag, got, c, ref=None, absum=None, rows=None):
    """Print e, e32 and B of the case and hold e to both gates; returns (ref, absum, B)."""
    if ref is None:
        ref, absum = V.vfe_net(c["vox"], c["num"], c["layers"], c["wd"])
    e32 = V.e32(c["vox"], c["num"], c["layers"], c["wd"], ref, absum)
    B = V.bound(c["T"], C.widths(c["layers"]))
    assert got.shape == ref.shape and np.isfinite(got).all()
    e = V.err(got, ref, absum)
    print(f"{tag}: e = {e:.3e}, e32 = {e32:.3e}, 3 e32 + 1e-8 = {V.gate(e32):.3e}, B = {B:.3e}")
    assert e <= B, f"{tag}: e = {e:.3e} > B = {B:.3e}"
    assert e <= V.gate(e32), f"{tag}: e = {e:.3e} > 3 e32 + 1e-8 = {V.gate(e32):.3e} (e32 = {e32:.3e})"
    return ref, absum, B


# ---------------------------------------------------------------- a. sizes
@pytest.mark.parametrize("F,wd,filters", C.SIZES)
def test_sizes_match_fp64(F, wd, filters):
    """Every F with and without the distance column (K1 = 6, 7, 8, 9, 13, 14: zero-padded weight rows wherever K1 is no
    multiple of 4), every accepted width of either VFE layer -- 48 units, the one width where the lane groups leave lanes
    idle, with padded weight rows and without."""
    c = C.size_case(F, wd, filters)
    K1, K1p = C.launch_shape(c["T"], F, wd, filters)[3:]
    got = _net(c).rows(*_dev(c["vox"], c["num"])).cpu().numpy()
    _gates(f"F {F} wd {wd} {filters} (K1 {K1}, K1p {K1p})", got, c)
    assert not got[0].any()                                       # count 0


# ---------------------------------------------------------------- b. every count
@pytest.mark.parametrize("T,filters", C.COUNT_RUNS)
def test_every_count_matches_fp64(T, filters):
    """T = 17: n = 0..17 four times over in shuffled order, so each row chunk of 8 or 4 ends full, one short and one over
    in both the layers that compute n rows and vfe1, which computes n + 1; T = 64: n = 0, 1, 63, 64."""
    c = C.count_case(T, filters)
    got = _net(c).rows(*_dev(c["vox"], c["num"])).cpu().numpy()
    ref, absum, B = _gates(f"T {T} {filters}", got, c)
    for n in sorted(set(c["num"].tolist())):                      # and per count, so a miss names its n
        sel = c["num"] == n
        assert V.err(got[sel], ref[sel], absum[sel]) <= B, f"n = {n}"
    assert not got[c["num"] == 0].any()


# ---------------------------------------------------------------- c. LDS launch shapes
@pytest.mark.parametrize("args,shape", C.LDS_SHAPES, ids=[f"V{v}_wpb{w}" for _, (v, w) in C.LDS_SHAPES])
def test_each_lds_shape_matches_fp64(args, shape):
    """One case per rung of the launcher's ladder -- (V, wpb) = (16,8), (2,8), (1,8), (1,4), (1,2), (1,1), the last the
    largest shape it accepts -- at M = 1 and M = 70."""
    T, F, wd, filters, vpw = args
    for M in C.LDS_M:
        c = C.lds_case(T, F, wd, filters, M)
        net, d = _net(c), _dev(c["vox"], c["num"])
        got = net.rows(*d, voxels_per_wave=vpw) if vpw else net.rows(*d)
        _gates(f"(V, wpb) = {shape} T {T} F {F} wd {wd} {filters} M {M}", got.cpu().numpy(), c)
        if vpw:
            assert torch.equal(_bits(got), _bits(net.rows(*d)))


@pytest.mark.parametrize("T,F,wd,filters", C.VPW16_RUNS)
def test_voxels_per_wave_16_gives_the_default_launch_bits(T, F, wd, filters):
    """voxels_per_wave = 16 (V = 16 twice, once within 4 KB of the LDS limit, and V = 8 after shrinking) around the
    group size: M = 1, 15, 16, 17, 129, one workgroup and as many as fit."""
    c = C.lds_case(T, F, wd, filters, max(C.VPW16_M))
    net = _net(c)
    for M in C.VPW16_M:
        d = _dev(c["vox"][:M], c["num"][:M])
        base = net.rows(*d)
        assert tuple(base.shape) == (M, filters[-1])
        for blocks in (1, 0):
            out = net.rows(*d, voxels_per_wave=16, max_blocks=blocks)
            assert torch.equal(_bits(out), _bits(base)), (M, blocks)
    _gates(f"vpw 16 T {T} {filters}", net.rows(*_dev(c["vox"], c["num"]), voxels_per_wave=16).cpu().numpy(), c)


# ---------------------------------------------------------------- d. counts outside [0, T]
def test_num_points_outside_the_slots_are_clipped():
    """-1 and -2^31 count as 0, T + 1 and 2^31 - 1 as T: the same bits as the clipped counts give, whatever the slots of
    a voxel with a count below 0 hold."""
    T = 10
    c = C.case(T, 5, 1, [32, 128], 70, counts=np.random.default_rng(4).integers(1, T + 1, size=70), seed=4)
    raw = c["num"].copy()
    raw[[3, 17, 40, 66]] = [-1, -2 ** 31, T + 1, 2 ** 31 - 1]
    vox = c["vox"].copy()
    for m in (3, 17, 40, 66):                                     # all T slots hold points
        vox[m] = vox[(m + 1) % 70, 0] + np.arange(T, dtype=np.float32)[:, None] * 0.01
    clipped = np.clip(raw.astype(np.int64), 0, T).astype(np.int32)
    assert clipped[[3, 17, 40, 66]].tolist() == [0, 0, T, T]
    net = _net(c)
    got = net.rows(*_dev(vox, raw))
    assert torch.equal(_bits(got), _bits(net.rows(*_dev(vox, clipped))))
    assert not got[[3, 17]].any()
    c2 = dict(c, vox=vox, num=raw)
    _gates("clipped counts", got.cpu().numpy(), c2)


# ---------------------------------------------------------------- e. the padded slots of the second VFE layer
def test_padded_slot_wins_vfe2_max():
    """The fixture (vfe_cases.vfe2_pad_fixture): b2 in 1..3, every w2 weight negative, so wherever n < T the padded slots'
    relu(b2) is vfe2's max.  A kernel that runs that max over the real rows only computes the other restatement."""
    c = C.vfe2_pad_fixture()
    h, _ = C.hidden_rows(c, 1)
    b2 = c["layers"][1][2]
    part = c["num"] < c["T"]
    for m in np.flatnonzero(part):                                # the claim about the fixture itself
        assert (h[m, :c["num"][m]] <= b2).all() and np.array_equal(h[m, c["num"][m]], b2)
    got = _net(c).rows(*_dev(c["vox"], c["num"])).cpu().numpy()
    ref, absum, B = _gates("vfe2 pad join", got, c)
    wrong, _ = V.vfe_net(c["vox"], c["num"], c["layers"], False, pad_in_max2=False)
    assert (np.abs(got - wrong) > 10 * B * absum).any(1)[part].all()


# ---------------------------------------------------------------- f. non-finite input
@pytest.mark.parametrize("filters", C.NAN_FILTERS)
def test_nan_voxel_rows_follow_the_documented_rule(filters):
    """csrc/vfe.hip: ReLU is fmaxf(pre, 0), so a NaN pre-activation gives 0.  A NaN in a feature past xyz zeroes its own
    slot's vfe1 row; a NaN coordinate makes the mean NaN, which zeroes every real slot's vfe1 row and the padded
    representative's.  The affected rows are finite and equal vfe_net(nan_rule=True) within B; every other voxel keeps
    the bits of the clean run.  (The reference gives NaN rows.)"""
    for wd in (False, True):
        c, clean, hit = C.nan_case(filters, wd)
        net = _net(c)
        got_t, clean_t = net.rows(*_dev(c["vox"], c["num"])), net.rows(*_dev(clean, c["num"]))
        got = got_t.cpu().numpy()
        ref, absum = V.vfe_net(c["vox"], c["num"], c["layers"], wd, nan_rule=True)
        B = V.bound(c["T"], C.widths(c["layers"]))
        assert np.isfinite(got).all()
        for m in hit:
            e = V.err(got[m], ref[m], absum[m])
            print(f"{filters} wd {wd} voxel {m}: e = {e:.3e}, B = {B:.3e}")
            assert e <= B, (m, e)
        assert V.err(got, ref, absum) <= B
        keep = torch.from_numpy(np.setdiff1d(np.arange(len(c["num"])), hit)).cuda()
        assert torch.equal(_bits(got_t[keep]), _bits(clean_t[keep]))
        assert not torch.equal(_bits(got_t[hit]), _bits(clean_t[hit]))
        assert torch.equal(_bits(got_t[20]), _bits(got_t[33]))    # both as if vfe1 had given 0: the same row


# ---------------------------------------------------------------- g. refusals
def _raw(fn, a, **kw):
    """Call ``fn`` through lib.call on raw pointers: ``a`` holds the good arguments, ``kw`` replaces some."""
    from al3d import lib
    a = dict(a, **kw)
    args = [a["vox"], a["num"], a["M"], a["T"], a["F"], a["wd"], a["w1"], a["s1"], a["b1"], a["U1"], a["w2"], a["s2"],
            a["b2"], a["U2"], a["w3"], a["s3"], a["b3"], a["C"], a["out"]]
    if fn == ENTRY_LAUNCH:
        args += [a.get("vpw", 0), a.get("blocks", 0)]
    lib.call(fn, *args, None)


def test_refusals_name_the_entry_point_and_write_nothing():
    from al3d import lib
    so = lib.load()
    c = C.case(10, 5, 0, [32, 128], 4, counts=np.array([1, 10, 4, 0]))
    net = _net(c)
    vox, num = _dev(c["vox"], c["num"])
    out = torch.full((4, 128), -7.5, device="cuda")
    (w1, s1, b1, u1), (w2, s2, b2, u2), (w3, s3, b3, cc) = net.packs
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(vox=p(vox), num=p(num), M=4, T=10, F=5, wd=0, w1=p(w1), s1=p(s1), b1=p(b1), U1=u1, w2=p(w2), s2=p(s2),
                b2=p(b2), U2=u2, w3=p(w3), s3=p(s3), b3=p(b3), C=cc, out=p(out))
    one = dict(good, w2=None, s2=None, b2=None, U2=0)            # one VFE layer of 16 units would give C = 32
    bad = [dict(T=0), dict(T=65), dict(F=2), dict(F=11), dict(U1=0), dict(U1=8), dict(U1=24), dict(U1=80), dict(U2=80),
           dict(C=64), dict(C=130), dict(M=-1), dict(w1=None), dict(s3=None), dict(b1=None), dict(vox=None),
           dict(num=None), dict(out=None), dict(s2=None)]
    for kw in bad:
        for fn in (ENTRY, ENTRY_LAUNCH):
            with pytest.raises(lib.Al3dError):
                _raw(fn, good, **kw)
            assert so.al3d_last_error().decode().startswith(fn + ":"), (kw, so.al3d_last_error())
    with pytest.raises(lib.Al3dError, match="twice the last VFE layer"):
        _raw(ENTRY, one, C=128)                                   # C != 2 * last units, one VFE layer
    for kw in (dict(vpw=-1), dict(vpw=17), dict(blocks=-1)):
        with pytest.raises(lib.Al3dError, match="launch shape"):
            _raw(ENTRY_LAUNCH, good, **kw)
        assert so.al3d_last_error().decode().startswith(ENTRY_LAUNCH + ":")
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())
    # M = 0 with null data pointers launches nothing and succeeds
    for fn in (ENTRY, ENTRY_LAUNCH):
        _raw(fn, good, M=0, vox=None, num=None, out=None)
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())
    # and the good arguments do run: the module's bits
    _raw(ENTRY, good)
    assert torch.equal(_bits(out), _bits(net.rows(vox, num)))
