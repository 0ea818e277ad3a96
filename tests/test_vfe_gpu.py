"""GPU suite: the fused VFE reader (csrc/vfe.hip) through the reader modules, against the float64 restatement
(tests/vfe_fp64.py) and the reference's own outputs (tests/golden/vfe_readers.npz).

Accuracy: e = max |got - ref64| / absum, absum the abs chain through decoration and all layers (vfe_fp64.vfe_net).  The
bound is the first-order worst case of the f32 chains, not a measured number: B = 1.25 * (T + K1 + K2 + K3 + 5) * 2^-24
with K_l the layers' input widths (vfe_fp64.bound): every dot of length K rounds at most K times plus the fold FMA, the
mean at most T + 1 times, the subtraction once; ReLU and max are exact; 1.25 covers the second-order terms.

Beside B, the tight gate e <= 3 e32 + 1e-8: e32 is the largest error of three float32 evaluations of the same formula on
the same case (vfe_fp64.e32, computed on the host, never from the kernel); factor and floor are the split rule of
tests/test_spconv_fp64_gpu.py.  B alone lets a kernel thousands of times less accurate than float32 through."""
import os

import numpy as np
import pytest
import torch

import vfe_fp64 as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "vfe_readers.npz"))
CASES = [str(c) for c in G["cases"]]


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _reader(kind, filters, use_norm, wd, F, params):
    from al3d.models import build_reader
    mod = build_reader(dict(type="VoxelFeatureExtractor" if kind == "vfe" else "VoxelFeatureExtractorV2",
                            num_input_features=F, use_norm=use_norm, num_filters=list(filters), with_distance=wd))
    sd = mod.state_dict()
    sd.update({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    mod.load_state_dict(sd, strict=True)
    return mod.cuda().eval()


def _widths(layers):
    return [w.shape[1] for w, _, _ in layers]


def _err(got, ref, absum):
    return float((np.abs(got.astype(np.float64) - ref) / absum).max()) if ref.size else 0.0


def _tight(tag, e, vox, num, layers, wd, ref, absum):
    e32 = V.e32(vox, num, layers, wd, ref, absum)
    print(f"{tag}: e = {e:.3e}, e32 = {e32:.3e}, 3 e32 + 1e-8 = {V.gate(e32):.3e}")
    assert e <= V.gate(e32), f"{tag}: e = {e:.3e} > 3 e32 + 1e-8 = {V.gate(e32):.3e} (e32 = {e32:.3e})"


# ---------------------------------------------------------------- the reference's own outputs
def _golden(tag):
    c = [int(v) for v in G[f"{tag}.config"]]
    cfg = dict(kind=tag.split("_")[0], use_norm=bool(c[0]), wd=bool(c[1]), F=c[2], T=c[3], filters=c[4:])
    pre = tag + "."
    params = {k[len(pre):]: G[k] for k in G.files
              if k.startswith(pre) and k[len(pre):] not in ("out", "keys", "shapes", "config")}
    if cfg["kind"] == "vfe":
        prefixes = [("vfe1.linear", "vfe1.norm"), ("vfe2.linear", "vfe2.norm"), ("linear", "norm")]
    else:
        prefixes = [(f"vfe_layers.{i}.linear", f"vfe_layers.{i}.norm") for i in range(len(cfg["filters"]))]
        prefixes.append(("linear", "norm"))
    return cfg, params, prefixes


@pytest.mark.parametrize("tag", CASES)
def test_module_matches_reference_and_fp64(tag):
    cfg, params, prefixes = _golden(tag)
    vox, num = G[f"voxels_F{cfg['F']}_T{cfg['T']}"], G[f"num_points_F{cfg['F']}_T{cfg['T']}"]
    mod = _reader(cfg["kind"], cfg["filters"], cfg["use_norm"], cfg["wd"], cfg["F"], params)
    got = mod(*_dev(vox, num)).cpu().numpy()
    layers = V.fold_layers(params, prefixes)
    ref, absum = V.vfe_net(vox, num, layers, cfg["wd"])
    B = V.bound(cfg["T"], _widths(layers))
    e = _err(got, ref, absum)
    print(f"{tag}: e = {e:.3e}, B = {B:.3e}")
    assert got.shape == ref.shape
    assert e <= B, f"e = {e:.3e} > B = {B:.3e}"
    _tight(tag, e, vox, num, layers, cfg["wd"], ref, absum)
    assert (np.abs(got - G[f"{tag}.out"]) <= 2 * B * absum).all()


# ---------------------------------------------------------------- seeded cases
def _seeded(T, F, filters, scale, M=257, seed=0, use_norm=True, wd=False):
    rng = np.random.default_rng(1000 * T + 10 * F + len(filters) + sum(filters) + seed)
    counts = rng.integers(1, T + 1, size=M)
    edge = [0, 1, T - 1, T, T + 1, T + 9]
    counts[:len(edge)] = edge[:M]
    vox, num = V.make_case(rng, M, T, F, counts=counts, scale=scale)
    params, prefixes = V.make_layers(rng, F + 3 + int(wd), filters, use_norm)
    mod = _reader("v2", filters, use_norm, wd, F, params)
    return vox, num, mod, V.fold_layers(params, prefixes)


@pytest.mark.parametrize("scale", [1e-4, 1.0, 300.0])
@pytest.mark.parametrize("filters", [[32, 128], [32, 64], [64]])
@pytest.mark.parametrize("T", [1, 5, 10, 33])
def test_kernel_matches_fp64(T, filters, scale):
    """M = 257 (a ragged last workgroup) with counts 0, 1, T - 1, T and above T among them; M = 0, 1, 3 are the first rows
    of the same voxels and must give the same bits."""
    for F in (4, 5):
        vox, num, mod, layers = _seeded(T, F, filters, scale, wd=F == 4)
        got_t = mod(*_dev(vox, num))
        got = got_t.cpu().numpy()
        ref, absum = V.vfe_net(vox, num, layers, F == 4)
        B = V.bound(T, _widths(layers))
        e = _err(got, ref, absum)
        print(f"T {T} F {F} filters {filters} scale {scale}: e = {e:.3e}, B = {B:.3e}")
        assert got.shape == ref.shape == (257, filters[-1])
        assert e <= B, f"F {F}: e = {e:.3e} > B = {B:.3e}"
        _tight(f"T {T} F {F} filters {filters} scale {scale}", e, vox, num, layers, F == 4, ref, absum)
        assert not got[0].any()                                   # count 0: every slot padded, the row is 0
        for m in (0, 1, 3):
            sub = mod(*_dev(vox[:m], num[:m]))
            assert tuple(sub.shape) == (m, filters[-1])
            assert torch.equal(_bits(sub), _bits(got_t[:m]))


def test_use_norm_false_matches_fp64():
    vox, num, mod, layers = _seeded(10, 5, [32, 128], 1.0, use_norm=False, wd=True, seed=5)
    assert "linear.bias" in mod.state_dict() and "norm.weight" not in mod.state_dict()
    got = mod(*_dev(vox, num)).cpu().numpy()
    ref, absum = V.vfe_net(vox, num, layers, True)
    e = _err(got, ref, absum)
    assert e <= V.bound(10, _widths(layers))
    _tight("use_norm=False", e, vox, num, layers, True, ref, absum)


def test_padded_slot_wins_vfe1_max():
    """n = 1 of 10 with a mean far from zero: the padded slots' [0..0, -mean] rows win vfe1's max for most units.  A
    kernel that masks them in front of vfe1 (PillarFeatureNet's order) computes the other restatement."""
    T, F, filters = 10, 5, [32, 128]
    rng = np.random.default_rng(77)
    vox, num = V.make_case(rng, 64, T, F, counts=np.ones(64, np.int64))
    params, prefixes = V.make_layers(rng, F + 3, filters)
    # the voxels lie around (-40, 30, -2): with vfe1's weights on xyz - mean signed (+, -, +) the padded slots' -mean
    # gives every unit a large positive sum; the raw xyz weights are scaled down so the one real point stays below it
    w1 = params["vfe_layers.0.linear.weight"]
    w1[:, F:F + 3] = np.abs(w1[:, F:F + 3]) * np.array([1.0, -1.0, 1.0], np.float32)
    w1[:, :3] *= 0.1
    layers = V.fold_layers(params, prefixes)
    # the claim about the fixture itself: a padded slot wins for most of vfe1's units
    w, s, b = layers[0]
    x = np.concatenate([vox[:, 0].astype(np.float64), np.zeros((64, 3))], 1)          # one point: xyz - mean = 0
    mean = vox[:, 0, :3].astype(np.float64)
    pad = np.concatenate([np.zeros((64, F)), -mean], 1)
    h_real, h_pad = np.maximum(x @ w.T * s + b, 0), np.maximum(pad @ w.T * s + b, 0)
    assert (h_pad > h_real).mean() > 0.5
    mod = _reader("v2", filters, True, False, F, params)
    got = mod(*_dev(vox, num)).cpu().numpy()
    ref, absum = V.vfe_net(vox, num, layers, False)
    wrong, _ = V.vfe_net(vox, num, layers, False, pad_in_max1=False)
    B = V.bound(T, _widths(layers))
    assert _err(got, ref, absum) <= B
    assert (np.abs(got - wrong) > 10 * B * absum).any()


def test_bits_do_not_depend_on_launch_shape_order_or_run():
    for T, filters in ((10, [32, 128]), (33, [32, 64]), (5, [64])):
        vox, num, mod, _ = _seeded(T, 5, filters, 1.0, seed=9)
        d = _dev(vox, num)
        net = mod.net(torch.device("cuda"))
        base = net.rows(*d)
        assert torch.equal(_bits(base), _bits(net.rows(*d)))                     # two runs
        for vpw in (1, 2, 0):
            for blocks in (1, 3, 0):
                out = net.rows(*d, voxels_per_wave=vpw, max_blocks=blocks)
                assert torch.equal(_bits(out), _bits(base)), (T, filters, vpw, blocks)
        out = net.rows(*d, voxels_per_wave=5, max_blocks=7)
        assert torch.equal(_bits(out), _bits(base))
        perm = torch.from_numpy(np.random.default_rng(3).permutation(len(num))).cuda()
        out = net.rows(d[0][perm], d[1][perm])
        assert torch.equal(_bits(out), _bits(base[perm]))


def test_non_finite_points_stay_in_their_voxel():
    vox, num, mod, _ = _seeded(10, 5, [32, 128], 1.0, seed=11)
    clean = mod(*_dev(vox, num))
    bad = vox.copy()
    i, j = 40, 131                                   # different waves, both with at least one point
    assert num[i] >= 1 and num[j] >= 1
    bad[i, 0, 1] = np.nan
    bad[j, 0, 3] = np.inf
    got = mod(*_dev(bad, num))
    keep = np.ones(len(num), bool)
    keep[[i, j]] = False
    keep = torch.from_numpy(keep).cuda()
    assert torch.equal(_bits(got[keep]), _bits(clean[keep]))


# ---------------------------------------------------------------- the two small readers
@pytest.mark.parametrize("T", [1, 5, 10])
@pytest.mark.parametrize("F", [4, 5])
def test_simple_voxel_and_ablation_match_reference(F, T):
    """<= 4 * 2^-24 relative to |sum| / n: a sum of at most T terms and one division."""
    from al3d.models import build_reader
    vox, num = G[f"voxels_F{F}_T{T}"], G[f"num_points_F{F}_T{T}"]
    d = _dev(vox, num)
    amean = np.abs(vox.astype(np.float64)).sum(1) / num[:, None]
    tol = 4 * 2.0 ** -24
    got = build_reader(dict(type="SimpleVoxel", num_input_features=F)).cuda()(*d).cpu().numpy()
    ref = G[f"simple_F{F}_T{T}.out"]
    size = np.concatenate([np.hypot(amean[:, 0], amean[:, 1])[:, None], amean[:, 2:F]], 1)
    assert got.shape == ref.shape == (len(num), F - 1)
    print(f"SimpleVoxel F {F} T {T}: {(np.abs(got - ref) / size).max() / 2.0 ** -24:.2f} x 2^-24")
    assert (np.abs(got - ref) <= tol * size).all()
    got = build_reader(dict(type="VFEV3_ablation", num_input_features=F)).cuda()(*d).cpu().numpy()
    ref = G[f"ablation_F{F}_T{T}.out"]
    size = np.concatenate([amean[:, [0, 1, 3]], 1.0 / num[:, None]], 1)
    assert got.shape == ref.shape == (len(num), 4)
    print(f"VFEV3_ablation F {F} T {T}: {(np.abs(got - ref) / size).max() / 2.0 ** -24:.2f} x 2^-24")
    assert (np.abs(got - ref) <= tol * size).all()
