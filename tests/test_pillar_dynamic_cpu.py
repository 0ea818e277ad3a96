"""CPU suite: the dynamic pillar net's float64 restatement (tests/pillar_dynamic_numpy.py) against the golden recorded from
the reference's own PillarFeatureNets on clouds whose pillars are all exactly full (tools/gen_golden_pillar_dynamic.py ->
tests/golden/pillar_dynamic.npz), and the Python surface: config, registry, state-dict keys, ABI names, the two guards."""
import os

import numpy as np
import pytest

import pillar_dynamic_numpy as RD
import pillars_fp64 as R
from test_pointpillars_golden import golden_geom, golden_layers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "pillar_dynamic.npz")
CONFIG = os.path.join(ROOT, "examples", "active", "bevfusion_pointpillars_dynamic_spatial_temporal_feature.py")
TAGS = ["f1_d0", "f1_d1", "f2_d0", "f2_d1"]


def golden():
    return np.load(G)


def golden_rows(g):
    """(point2voxel, coords, mean) of the golden's shuffled points, with the rows in the golden's coordinate order."""
    p2v, coords, mean = RD.voxelize(g["points"], g["point_offsets"], g["pc_range"], g["voxel_size"], g["grid"])
    assert np.array_equal(coords, g["coords"])          # both ascending in (b, y, x)
    return p2v, coords, mean


def test_golden_fixture_shape():
    g = golden()
    assert "factory stand-ins" in str(g["standin"])
    assert os.path.getsize(G) < 512 * 1024
    M, P, F = g["voxels"].shape
    assert (g["num_points"] == P).all() and P == 4 and F == 5       # no padded slot, no truncation
    nx, ny, B = [int(v) for v in g["grid"]]
    assert nx != ny
    c = g["coords"]
    assert set(np.unique(c[:, 0])) == {0, 2}                        # frame 1 is empty
    assert (c[:, 3] == 0).any() and (c[:, 3] == nx - 1).any() and (c[:, 2] == 0).any() and (c[:, 2] == ny - 1).any()
    assert list(g["cases"]) == TAGS
    assert len(g["points"]) == M * P and int(g["point_offsets"][-1]) == M * P
    # shuffled: the points of a pillar are not consecutive
    p2v, _, _ = golden_rows(g)
    assert (np.bincount(p2v, minlength=M) == P).all() and (np.diff(p2v) != 0).mean() > 0.9
    # the slots hold each pillar's points in ascending point index
    for r in (0, M // 2, M - 1):
        assert np.array_equal(g["voxels"][r], g["points"][np.flatnonzero(p2v == r)])


@pytest.mark.parametrize("tag", TAGS)
def test_fp64_restatement_matches_reference_pillar_nets(tag):
    """Both reference PillarFeatureNets on full slots are the expected output of a net over all points; the bound is the
    one tests/test_pointpillars_golden.py holds its own restatement to."""
    g = golden()
    layers, geom = golden_layers(g, tag), golden_geom(g, tag)
    p2v, coords, _ = golden_rows(g)
    ref, absum = RD.pfn_dynamic(g["points"], p2v, coords, layers, *geom)
    bev, _ = RD.pfn_dynamic(g["points"], p2v, coords[:, [0, 3, 2, 1]], layers, *geom, xcol=1, ycol=2)
    for want, got in ((g[f"{tag}.out_det3d"], ref), (g[f"{tag}.out_bevfusion"], bev)):
        assert want.shape == got.shape
        e = float((np.abs(want.astype(np.float64) - got) / absum).max())
        print(f"{tag}: e = {e:.3e}")
        assert e <= 2e-6, f"{tag}: e = {e:.3e}"                      # the reference ran in float32


@pytest.mark.parametrize("tag", ["f1_d1", "f2_d0"])
def test_restatement_equals_the_slot_restatement_on_full_pillars(tag):
    """Without padded slots the two float64 restatements state the same function."""
    g = golden()
    layers, geom = golden_layers(g, tag), golden_geom(g, tag)
    p2v, coords, _ = golden_rows(g)
    dyn, _ = RD.pfn_dynamic(g["points"], p2v, coords, layers, *geom)
    hard, _ = R.pfn_net(g["voxels"], g["num_points"], coords, layers, *geom)
    assert float(np.abs(dyn - hard).max()) <= 1e-12 * max(1.0, float(np.abs(hard).max()))


def test_restatement_drops_the_padded_slot_floor():
    """The one deliberate difference: a partly filled hard pillar also pools relu(shift1); the dynamic net does not."""
    rng = np.random.default_rng(5)
    vox, n, coords = R.make_case(rng, 40, 8, counts=rng.integers(1, 8, 40))
    raw = R.make_layers(rng, 10, [32])
    layers = [(w, *R.fold_bn(g_, b_, m_, v_, eps)) for w, g_, b_, m_, v_, eps in raw]
    geom = (0.2, 0.2, 0.1 - 51.2, 0.1 - 51.2, False)
    pts = np.concatenate([vox[i, :n[i]] for i in range(40)])
    p2v = np.repeat(np.arange(40), n)
    dyn, _ = RD.pfn_dynamic(pts, p2v, coords, layers, *geom)
    hard, _ = R.pfn_net(vox, n, coords, layers, *geom)
    floor = np.maximum(layers[0][2], 0.0)
    assert np.allclose(hard, np.maximum(dyn, floor[None]), rtol=0, atol=1e-12)
    assert (dyn < hard).any()


def test_example_config_builds_and_names_the_dynamic_reader():
    from al3d import detector_ops as D
    from al3d.models import READERS, DynamicPillarFeatureNet, PillarFeatureNet, build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(CONFIG)
    vg = cfg.voxel_generator
    assert vg.max_points_in_voxel == -1 and vg.max_voxel_num == -1 and D.voxelizer_class(vg) is D.DynamicVoxelizer
    hard = Config.fromfile(CONFIG.replace("_dynamic", ""))
    assert list(vg.range) == list(hard.voxel_generator.range) and list(vg.voxel_size) == list(hard.voxel_generator.voxel_size)
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    assert type(m.reader) is DynamicPillarFeatureNet and m.bbox_head is None
    assert READERS.get("DynamicPillarFeatureNet") is DynamicPillarFeatureNet
    h = build_detector(hard.model, train_cfg=None, test_cfg=hard.test_cfg)
    assert type(h.reader) is PillarFeatureNet
    # same parameter names and shapes: a PointPillars checkpoint loads into either, strict
    assert list(m.reader.state_dict()) == list(h.reader.state_dict())
    assert "pfn_layers.1.linear.weight" in m.reader.state_dict() and "pfn_layers.0.norm.running_var" in m.reader.state_dict()
    missing, unexpected = m.load_state_dict(h.state_dict(), strict=True)
    assert not missing and not unexpected
    assert m.prepare({}) is None


def test_abi_names_resolve():
    from al3d import lib
    so = lib.load()
    for name in ("al3d_pillar_net_dynamic_workspace_bytes", "al3d_pillar_net_dynamic_f32",
                 "al3d_pillar_net_dynamic_launch_f32"):
        assert name in lib.SIGNATURES and hasattr(so, name)
    assert so.al3d_pillar_net_dynamic_workspace_bytes(1000, 64, 0) == 0             # one layer pools into the output
    two = so.al3d_pillar_net_dynamic_workspace_bytes(1000, 64, 1)
    assert two >= 1000 * 64 * 4 and so.al3d_pillar_net_dynamic_workspace_bytes(0, 64, 1) == 0
    # argument checks come before any launch
    rc = so.al3d_pillar_net_dynamic_f32(None, None, 0, 2, None, 3, None, 0, 0.2, 0.2, 0.1, 0.1, 0, None, None, None, 64,
                                        None, None, None, 0, 1, 4, 4, None, 0, None, None, None)
    assert rc == -1 and b"3 <= F <= 10" in so.al3d_last_error()
    rc = so.al3d_pillar_net_dynamic_f32(None, None, 0, 5, None, 3, None, 0, 0.2, 0.2, 0.1, 0.1, 0, 8, 8, 8, 24,
                                        None, None, None, 0, 1, 4, 4, None, 0, None, None, None)
    assert rc == -1 and b"multiple of 16" in so.al3d_last_error()


def test_hard_only_guards_still_raise():
    from al3d import detector_ops as D
    base = dict(range=[-4, -4, -2, 4, 4, 2], voxel_size=[0.5, 0.5, 1.0], max_points_in_voxel=-1, max_voxel_num=-1)
    with pytest.raises(NotImplementedError, match="dynamic pillar") as e:
        D.build_voxelizer(base, 1, "cpu", with_points=True)
    assert "keep_points=True" in str(e.value)
    vox = D.build_voxelizer(base, 1, "cpu")
    with pytest.raises(NotImplementedError, match="dynamic pillar"):
        vox(None, None, want_voxels=True)


def test_pointpillars_names_keep_points_when_the_points_are_missing():
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(CONFIG)
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg).eval()
    ex = dict(voxel_features=None, coordinates=None, num_voxels=[0], shape=np.array([[512, 512, 1]]))
    with pytest.raises(RuntimeError, match="keep_points=True"):
        m.sparse_stage(ex)
