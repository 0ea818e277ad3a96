"""GPU suite: dynamic voxelization (csrc/voxelize_dyn.hip) -- ``DynamicVoxelizer``, the ``Voxelization`` / ``DynamicScatter`` /
``dynamic_scatter`` mirror, the loaders and the lidar detector on it.  Comparisons are bitwise unless said otherwise: the
coordinates and counts are integers, the float32 sum runs in ascending point index on both sides (the golden fixture of
the reference's layers and the numpy yardstick tests/voxel_dynamic_numpy.py)."""
import os

import numpy as np
import pytest
import torch

import voxel_dynamic_numpy as Y

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DYN_CFG = os.path.join(ROOT, "examples", "active", "bevfusion_lidar_dynamic_spatial_temporal_feature.py")
RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]          # the hard voxelizer suite's grid: 1024 x 1024 x 40
VSIZE = [0.1, 0.1, 0.2]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def run_dyn(frames, pc_range, vsize, order="zyx", reduce="mean", extra_tail=None):
    from al3d import detector_ops as D
    vox = D.DynamicVoxelizer(pc_range, vsize, reduce=reduce, order=order, device=DEV)
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    parts = [f for f in frames if len(f)] + ([extra_tail] if extra_tail is not None else [])
    pts = np.concatenate(parts, axis=0) if parts else np.zeros((0, 5), np.float32)
    out = vox(torch.from_numpy(pts).to(DEV), torch.from_numpy(off).to(DEV), want_point_coords=True)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def check_against_yardstick(out, frames, pc_range, vsize, order, reduce):
    ref = Y.voxelize_batch(frames, pc_range, vsize, order, reduce)
    n = sum(len(f) for f in frames)
    assert np.array_equal(out["num_voxels"], ref["num_voxels"])
    assert np.array_equal(out["row_base"], np.concatenate([[0], np.cumsum(ref["num_voxels"])]))
    assert np.array_equal(out["coords"], ref["coords"])
    assert np.array_equal(out["num_points"], ref["counts"])
    assert np.array_equal(out["point2voxel"][:n], ref["point2voxel"])
    assert np.array_equal(_bits(out["feat"]), _bits(ref["feat"]))
    assert out["voxel_cap"] == max(1, int(ref["num_voxels"].max()))
    return ref


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "dynamic_voxel.npz"))
    off = z["offsets"]
    return z, [z["points"][off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.mark.parametrize("order", ["zyx", "xyz"])
@pytest.mark.parametrize("reduce", ["mean", "sum", "max"])
def test_fixture_through_the_dynamic_voxelizer(fx, order, reduce):
    z, frames = fx
    out = run_dyn(frames, z["pc_range"], z["voxel_size"], order, reduce)
    assert np.array_equal(out["coords"], z[f"{order}_{reduce}_coords"])
    assert np.array_equal(_bits(out["feat"]), _bits(z[f"{order}_{reduce}_feat"]))
    assert np.array_equal(out["point_coords"], z["point_coords"])
    if order == "zyx":
        assert np.array_equal(out["num_points"], z[f"zyx_{reduce}_counts"])
    check_against_yardstick(out, frames, z["pc_range"], z["voxel_size"], order, reduce)


def test_fixture_through_the_public_mirror(fx):
    """Voxelization(-1) + DynamicScatter with 3- and 4-column coors, and dynamic_scatter('sum')."""
    from al3d.models import DynamicScatter, Voxelization, dynamic_scatter
    z, frames = fx
    vox = Voxelization(z["voxel_size"].tolist(), z["pc_range"].tolist(), -1).eval()
    coors = [vox(torch.from_numpy(f).to(DEV)) for f in frames]
    assert coors[0].dtype == torch.int32 and coors[0].shape == (len(frames[0]), 3)
    assert np.array_equal(torch.cat(coors).cpu().numpy(), z["point_coords"])
    allpts = torch.from_numpy(z["points"]).to(DEV)
    batched = torch.cat([torch.nn.functional.pad(c, (1, 0), value=b) for b, c in enumerate(coors)])
    for avg, red in ((True, "mean"), (False, "max")):
        layer = DynamicScatter(z["voxel_size"].tolist(), z["pc_range"].tolist(), avg)
        f4, c4 = layer(allpts, batched)
        assert np.array_equal(c4.cpu().numpy(), z[f"xyz_{red}_coords"])
        assert np.array_equal(_bits(f4.cpu().numpy()), _bits(z[f"xyz_{red}_feat"]))
        per = [layer(torch.from_numpy(f).to(DEV), c) for f, c in zip(frames, coors)]
        assert torch.equal(torch.cat([p[0] for p in per]), f4)
        assert torch.equal(torch.cat([p[1] for p in per]), c4[:, 1:])
    f0, c0 = dynamic_scatter(torch.from_numpy(frames[0]).to(DEV), coors[0], "sum")
    m0 = int((z["xyz_sum_coords"][:, 0] == 0).sum())
    assert np.array_equal(c0.cpu().numpy(), z["xyz_sum_coords"][:m0, 1:])
    assert np.array_equal(_bits(f0.cpu().numpy()), _bits(z["xyz_sum_feat"][:m0]))
    # every row dropped, and no row at all
    none = torch.full((4, 3), -1, dtype=torch.int32, device=DEV)
    fe, ce = dynamic_scatter(torch.ones((4, 5), device=DEV), none, "max")
    assert fe.shape == (0, 5) and ce.shape == (0, 3)
    fe, ce = dynamic_scatter(torch.ones((0, 5), device=DEV), none[:0], "mean")
    assert fe.shape == (0, 5) and ce.shape == (0, 3)


def test_hard_voxelization_through_the_mirror(oracle):
    """With caps the mirror wraps the hard voxelizer for one frame: the reference's three tensors, (x, y, z) coordinates."""
    from al3d import synthetic
    from al3d.models import Voxelization
    pts = synthetic.make_point_cloud(31, nsweeps=1)
    layer = Voxelization(VSIZE, RANGE, 10, max_voxels=(9000, 7000)).eval()
    voxels, coors, num = layer(torch.from_numpy(pts).to(DEV))
    v, c, n, _ = oracle.voxelize(pts, RANGE[:3], VSIZE, [1024, 1024, 40], 10, 7000)
    assert np.array_equal(coors.cpu().numpy(), c[:, ::-1]) and np.array_equal(num.cpu().numpy(), n)
    assert np.array_equal(_bits(voxels.cpu().numpy()), _bits(v))


def _cell_point(rng, ix, iy, iz, k):
    base = np.array([RANGE[0] + 0.1 * ix, RANGE[1] + 0.1 * iy, RANGE[2] + 0.2 * iz], np.float32)
    jit = rng.uniform(0.01, 0.09, (k, 3)).astype(np.float32) * np.array([1, 1, 2], np.float32)
    return np.concatenate([base + jit, rng.uniform(0, 255, (k, 1)).astype(np.float32),
                           rng.uniform(0, 0.5, (k, 1)).astype(np.float32)], 1)


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_runs_frames_and_edges(reduce):
    """The wave-level aggregation (one bit atomic and one slot request per run of adjacent lanes in a cell) and the frame
    bookkeeping on the patterns that stress them; per frame against the yardstick, point2voxel and counts included."""
    rng = np.random.default_rng(3)
    a = _cell_point(rng, 500, 500, 10, 300)                                  # one cell, 300 points in a row
    b = np.stack([_cell_point(rng, 100 + (i % 2), 200, 5, 1)[0] for i in range(150)])   # two cells alternating
    c = np.concatenate([_cell_point(rng, 10 + i, 20, 3, int(r)) for i, r in enumerate(rng.integers(1, 7, 60))])
    d = _cell_point(rng, 700, 300, 20, 40)
    d[5:9, 0] = 1e4                                                          # out of range inside a run
    d[20, 1] = np.nan                                                        # a NaN inside a run
    f0 = np.concatenate([a, b, c, d]).astype(np.float32)                     # ends in mid-wave
    f1 = np.concatenate([_cell_point(rng, 500, 500, 10, 70), c[::-1], a[:33]]).astype(np.float32)
    far = np.full((37, 5), 1e4, np.float32)                                  # a frame entirely out of range
    edge = np.array([[RANGE[0], RANGE[1], RANGE[2], 1, 0],                   # exactly range_min: kept
                     [RANGE[3], 0, 0, 1, 0], [0, RANGE[4], 0, 1, 0], [0, 0, RANGE[5], 1, 0],   # exactly range_max: dropped
                     [0.05, 0.05, 0.05, -0.0, 0.0], [0.05, 0.05, 0.05, 0.0, -0.0],             # signed zeros in one cell
                     [7.05, 0.05, 0.05, -0.0, -0.0]], np.float32)
    empty = np.zeros((0, 5), np.float32)
    frames = [empty, f0, f1, empty, far, edge, _cell_point(rng, 1, 1, 1, 5), empty]
    out = run_dyn(frames, RANGE, VSIZE, "zyx", reduce)
    ref = check_against_yardstick(out, frames, RANGE, VSIZE, "zyx", reduce)
    assert ref["num_voxels"].tolist()[0] == 0 and ref["num_voxels"][3] == 0 and ref["num_voxels"][4] == 0
    assert ref["num_voxels"][5] == 3 and ref["counts"].max() == 300
    e0 = int(np.cumsum(ref["num_voxels"])[4])
    assert out["coords"][e0].tolist() == [5, 0, 0, 0]
    if reduce == "mean":
        assert _bits(out["feat"][e0 + 2, 3:]).tolist() == _bits(np.array([0.0, 0.0], np.float32)).tolist()   # 0.f + -0.f
    else:
        assert _bits(out["feat"][e0 + 2, 3:]).tolist() == _bits(np.array([-0.0, -0.0], np.float32)).tolist()
        assert not np.signbit(out["feat"][e0 + 1, 3:]).any()                 # -0.f < +0.f whatever the order


def test_points_past_the_last_offset_belong_to_no_frame():
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-50, 50, (3000, 2)), rng.uniform(-4, 2, (3000, 1)), rng.uniform(0, 1, (3000, 2))],
                         1).astype(np.float32)
    tail = rng.uniform(-50, 50, (700, 5)).astype(np.float32)
    frames = [pts[:1200], pts[1200:]]
    a = run_dyn(frames, RANGE, VSIZE)
    b = run_dyn(frames, RANGE, VSIZE, extra_tail=tail)
    for k in ("feat", "coords", "num_points", "num_voxels"):
        assert np.array_equal(a[k], b[k]), k
    assert np.all(b["point2voxel"][3000:] == -1) and np.all(b["point_coords"][3000:] == -1)
    assert np.array_equal(a["point2voxel"], b["point2voxel"][:3000])


def test_a_heavy_voxel_spanning_workgroups():
    """5,000 points of one cell spread among 2,000 scattered ones: the voxel's points sit in 28 workgroups of the point
    passes and its reduction takes the workgroup path; mean and sum equal the sequential float32 sum."""
    rng = np.random.default_rng(8)
    heavy = _cell_point(rng, 512, 300, 7, 5000)
    rest = np.concatenate([rng.uniform(-50, 50, (2000, 2)), rng.uniform(-4, 2, (2000, 1)), rng.uniform(0, 1, (2000, 2))],
                          1).astype(np.float32)
    pts = np.concatenate([heavy, rest])[rng.permutation(7000)]
    for reduce in ("mean", "sum", "max"):
        out = run_dyn([pts], RANGE, VSIZE, "zyx", reduce)
        ref = check_against_yardstick(out, [pts], RANGE, VSIZE, "zyx", reduce)
        assert ref["counts"].max() == 5000
    row = int(np.argmax(out["num_points"]))
    acc = np.zeros(5, np.float32)
    for i in np.flatnonzero(out["point2voxel"] == row):
        acc = acc + pts[i]
    assert np.array_equal(_bits(run_dyn([pts], RANGE, VSIZE, "zyx", "sum")["feat"][row]), _bits(acc))


def test_determinism_and_point_order():
    from al3d import synthetic
    rng = np.random.default_rng(9)
    frames = [synthetic.make_point_cloud(40, nsweeps=1), synthetic.make_point_cloud(41, nsweeps=2)]
    a, b = run_dyn(frames, RANGE, VSIZE), run_dyn(frames, RANGE, VSIZE)
    for k in ("feat", "coords", "num_points", "num_voxels", "point2voxel", "point_coords"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    shuffled = [f[rng.permutation(len(f))] for f in frames]
    m0, m1 = run_dyn(frames, RANGE, VSIZE, reduce="max"), run_dyn(shuffled, RANGE, VSIZE, reduce="max")
    for k in ("feat", "coords", "num_points", "num_voxels"):
        assert np.array_equal(_bits(m0[k]), _bits(m1[k])), k
    assert np.array_equal(a["coords"], m1["coords"]) and a["num_points"].max() > 10


def test_agreement_with_the_hard_voxelizer():
    """Where no cap bites (no voxel above 10 points, no frame above max_voxels) the hard voxelizer's rows, sorted by
    (b, z, y, x), are the dynamic rows: features, coordinates and counts bit for bit."""
    from al3d import detector_ops as D
    rng = np.random.default_rng(10)
    frames = []
    for n in (9000, 4000):
        p = np.concatenate([rng.uniform(-20, 20, (n, 2)), rng.uniform(-4, 2, (n, 1)), rng.uniform(0, 1, (n, 2))], 1)
        p[: n // 3] = p[n // 3: 2 * (n // 3)] + rng.uniform(0, 0.02, (n // 3, 5))       # pairs that share cells
        frames.append(p.astype(np.float32))
    dyn = run_dyn(frames, RANGE, VSIZE)
    assert 1 < dyn["num_points"].max() <= 10 and dyn["num_voxels"].max() < 9000
    hard = D.Voxelizer(RANGE, VSIZE, 10, 9000, max_batch=2, device=DEV)
    off = torch.tensor([0, 9000, 13000], dtype=torch.int64, device=DEV)
    h = hard(torch.from_numpy(np.concatenate(frames)).to(DEV), off)
    hc = h["coords"].cpu().numpy().astype(np.int64)
    perm = np.lexsort((hc[:, 3], hc[:, 2], hc[:, 1], hc[:, 0]))
    assert np.array_equal(hc[perm], dyn["coords"])
    assert np.array_equal(h["num_points"].cpu().numpy()[perm], dyn["num_points"])
    assert np.array_equal(_bits(h["feat"].cpu().numpy()[perm]), _bits(dyn["feat"]))


def test_the_real_grid():
    """1440 x 1440 x 41 at 0.075 / 0.2 m, two frames of 120,000 synthetic points: a frame above 65,535 voxels (the sparse
    encoder's per-frame sort limit) and keys above 2^26."""
    from al3d import synthetic
    rng_, vs = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.2], [0.075, 0.075, 0.2]
    assert Y.grid_of(rng_, vs).tolist() == [1440, 1440, 41]
    frames = []
    for i in range(2):                               # every other point of a 10-sweep frame; the second frame lifted by 0.9 m
        p = synthetic.make_point_cloud(60 + i, nsweeps=10)[::2][:120000].copy()
        p[:, 2] += np.float32(0.9 * i)
        frames.append(p)
    assert all(len(f) == 120000 for f in frames)
    out = run_dyn(frames, rng_, vs)
    ref = check_against_yardstick(out, frames, rng_, vs, "zyx", "mean")
    assert ref["num_voxels"].min() > 65535
    c = out["coords"].astype(np.int64)
    assert ((c[:, 1] * 1440 + c[:, 2]) * 1440 + c[:, 3]).max() > 2 ** 26
    x = run_dyn(frames, rng_, vs, order="xyz", reduce="max")
    check_against_yardstick(x, frames, rng_, vs, "xyz", "max")


def test_rows_cap_too_small_is_refused():
    from al3d import detector_ops as D, lib
    rng = np.random.default_rng(12)
    pts = np.concatenate([rng.uniform(-50, 50, (500, 2)), rng.uniform(-4, 2, (500, 1)), rng.uniform(0, 1, (500, 2))],
                         1).astype(np.float32)
    vox = D.DynamicVoxelizer(RANGE, VSIZE, device=DEV)
    off = torch.tensor([0, 500], dtype=torch.int64, device=DEV)
    full = vox(torch.from_numpy(pts).to(DEV), off)
    m = full["feat"].shape[0]
    assert m > 100
    with pytest.raises(lib.Al3dError, match="rows_cap"):
        vox(torch.from_numpy(pts).to(DEV), off, rows_cap=m - 1)
    again = vox(torch.from_numpy(pts).to(DEV), off, rows_cap=m)             # exactly enough
    assert torch.equal(again["feat"], full["feat"]) and torch.equal(again["coords"], full["coords"])


def _small_cfg():
    from al3d.utils import Config
    cfg = Config.fromfile(DYN_CFG)
    X, Yn, Z = 32, 48, 40                            # BEV 4 x 6 behind the encoder: even, as the neck's 2x deblock needs
    lo = np.array([-1.2, -1.8, -5.0])
    vg = dict(range=[lo[0], lo[1], lo[2], lo[0] + 0.075 * X, lo[1] + 0.075 * Yn, 3.0], voxel_size=[0.075, 0.075, 0.2],
              max_points_in_voxel=cfg.voxel_generator.max_points_in_voxel, max_voxel_num=cfg.voxel_generator.max_voxel_num)
    return cfg, vg, (X, Yn, Z)


def _small_frames(rng, n_frames, vg, n=2500):
    lo, hi = np.array(vg["range"][:3]), np.array(vg["range"][3:])
    out = []
    for _ in range(n_frames):
        p = np.concatenate([rng.uniform(lo - 0.05, hi + 0.05, (n, 3)), rng.uniform(0, 1, (n, 1)), rng.uniform(0, 0.45, (n, 1))],
                           1).astype(np.float32)
        p[:, 2] = np.minimum(p[:, 2], -1.0 + 0.5 * rng.standard_normal(n).astype(np.float32))
        out.append(p)
    return out


def test_dynamic_loader_feeds_the_lidar_detector():
    """The dynamic loader's rows through the lidar FPNVoxelNet's encoder against the dense torch emulation of the encoder
    fed the same rows (test_detector_gpu's whole-encoder comparison and tolerance); the rows are the yardstick's."""
    import copy
    from al3d import detector_ops as D
    from al3d.datasets import DeviceSweepLoader, PoolFrames
    from al3d.models import build_detector
    from al3d import synthetic
    from test_detector_gpu import _dense_encoder_reference
    cfg, vg, (X, Yn, Z) = _small_cfg()
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=3)
    model.eval()
    cpu_backbone = copy.deepcopy(model.backbone)
    model = model.to(DEV)
    frames = _small_frames(np.random.default_rng(14), 2, vg)
    loader = DeviceSweepLoader(PoolFrames.from_numpy(frames, DEV), vg, None, batch_size=2, device=DEV)
    assert isinstance(loader.voxelizer, D.DynamicVoxelizer)
    ex = next(iter(loader))
    ref = Y.voxelize_batch(frames, vg["range"], vg["voxel_size"], "zyx", "mean")
    feats, coords = ex["voxel_features"].cpu().numpy(), ex["coordinates"].cpu().numpy()
    assert np.array_equal(coords, ref["coords"]) and np.array_equal(_bits(feats), _bits(ref["feat"]))
    assert np.array_equal(ex["num_points"].cpu().numpy(), ref["counts"]) and ex["voxel_cap"] == int(ref["num_voxels"].max())
    assert list(ex["shape"][0]) == [X, Yn, Z]
    with torch.no_grad():
        out, _ = model.backbone(ex["voxel_features"], ex["coordinates"], 2, np.array([X, Yn, Z]),
                                **model._cap_kw(ex["voxel_cap"]))            # voxel_cap -> the encoder's frame_rows_max
    want = _dense_encoder_reference(cpu_backbone, feats, coords, 2, [Z + 1, Yn, X])
    assert out.shape == want.shape
    # 21 stacked fp32-class convs; activations are O(1): absolute tolerance dominates (test_sparse_encoder_vs_dense_torch)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-3, atol=2e-4)


def test_dynamic_sweep_and_the_pillar_refusal():
    from al3d import sweep as S, synthetic
    from al3d.datasets import DeviceSweepLoader, PoolFrames
    from al3d.models import build_detector
    cfg, vg, _ = _small_cfg()
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    model = model.to(DEV).eval()
    frames = _small_frames(np.random.default_rng(15), 5, vg)
    pool = PoolFrames.from_numpy(frames, DEV)
    loader = DeviceSweepLoader(pool, vg, None, batch_size=2, device=DEV)
    assert len(loader) == 3
    emb = S.sweep_embeddings(model, loader, DEV, len(pool))                  # detector(example, estimate=True) per batch
    assert emb.shape == (5, 512) and bool(torch.isfinite(emb).all()) and float(emb.abs().max()) > 0
    # the order of the points in a frame does not reach the embedding
    rng = np.random.default_rng(16)
    pool2 = PoolFrames.from_numpy([f[rng.permutation(len(f))] for f in frames], DEV)
    ex, ex2 = next(iter(loader)), next(iter(DeviceSweepLoader(pool2, vg, None, batch_size=2, device=DEV)))
    assert torch.equal(ex["coordinates"], ex2["coordinates"]) and torch.equal(ex["num_points"], ex2["num_points"])
    with pytest.raises(NotImplementedError, match="dynamic pillar"):
        DeviceSweepLoader(pool, vg, None, batch_size=2, device=DEV, with_points=True)


def test_cli_sweeps_a_synthetic_pool_with_the_dynamic_config(tmp_path):
    """tools/active_select.py with the dynamic example config at full size (0.075 m grid, no caps): bootstrap the empty
    buffer, then sweep + select."""
    import json
    import subprocess
    import sys
    cmd = [sys.executable, os.path.join(ROOT, "tools", "active_select.py"), "--config", DYN_CFG, "--budget", "20", "--pred",
           "--synthetic-scenes", "1", "--batch", "4"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for _ in range(2):
        r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    out = json.load(open(tmp_path / "data" / "buffers" / "bevfusion_lidar_dynamic_stf.json"))
    assert list(out) == ["0", "20"] and len(out["20"]) >= 1 and len(set(out["20"])) == len(out["20"])


def test_pipeline_stage_picks_the_dynamic_voxelizer(fx):
    """datasets/pipelines.Voxelization with caps of -1: the dynamic rows in the stage's reference-shaped dictionary (no
    padded slots), through the same selection function as the loaders."""
    from al3d.datasets.pipelines import Voxelization
    z, frames = fx
    stage = Voxelization(cfg=dict(range=z["pc_range"].tolist(), voxel_size=z["voxel_size"].tolist(),
                                  max_points_in_voxel=-1, max_voxel_num=-1), device=DEV)
    res, _ = stage({"lidar": {"points": frames[0], "combined": None}, "mode": "val"}, {})
    v = res["lidar"]["voxels"]
    m = int((z["zyx_mean_coords"][:, 0] == 0).sum())
    assert v["voxels"] is None and v["num_voxels"].tolist() == [m] and list(v["shape"]) == [12, 10, 4]
    assert np.array_equal(v["coordinates"].cpu().numpy(), z["zyx_mean_coords"][:m, 1:])
    assert np.array_equal(_bits(v["voxel_features"].cpu().numpy()), _bits(z["zyx_mean_feat"][:m]))
    assert np.array_equal(v["num_points"].cpu().numpy(), z["zyx_mean_counts"][:m])


def test_file_loader_builds_the_dynamic_voxelizer(tmp_path):
    """FileSweepLoader with the dynamic example config on a small on-disk pool (ragged last batch; the merged tensor may be
    longer than the last offset): the same example as DeviceSweepLoader on the same clouds, rows of the yardstick."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from write_synthetic_pool import write_pool
    from al3d import detector_ops as D
    from al3d.datasets import DeviceSweepLoader, FileSweepLoader, PoolFrames
    from al3d.utils import Config
    vg = Config.fromfile(DYN_CFG).voxel_generator
    root = str(tmp_path / "pool")
    infos, _ = write_pool(root, scenes=1, base=2, nsweeps=2)
    infos = infos[:3]
    loader = FileSweepLoader(infos, vg, None, batch_size=2, device=DEV, root=root, threads=2, depth=2, nsweeps=2)
    assert isinstance(loader.voxelizer, D.DynamicVoxelizer) and len(loader) == 2
    examples, clouds = [], []
    for ex in loader:
        off, pts = ex["point_offsets"].cpu().numpy(), ex["points"].cpu().numpy()
        clouds += [pts[off[b]:off[b + 1]] for b in range(len(off) - 1)]
        examples.append(ex)
    ref_ex = list(DeviceSweepLoader(PoolFrames.from_numpy(clouds, DEV), vg, None, batch_size=2, device=DEV))
    for a, b in zip(examples, ref_ex):
        for k in ("voxel_features", "coordinates", "num_points", "num_voxels"):
            assert torch.equal(a[k], b[k]), k
        assert a["voxel_cap"] == b["voxel_cap"] and a["voxel_cap"] == int(a["num_voxels"].max())
    ref = Y.voxelize_batch(clouds[:2], vg.range, vg.voxel_size, "zyx", "mean")
    assert np.array_equal(examples[0]["coordinates"].cpu().numpy(), ref["coords"])
    assert np.array_equal(_bits(examples[0]["voxel_features"].cpu().numpy()), _bits(ref["feat"]))
    with pytest.raises(NotImplementedError, match="dynamic pillar"):
        FileSweepLoader(infos, vg, None, batch_size=2, device=DEV, root=root, with_points=True)


@pytest.mark.parametrize("nfeat", [3, 4, 7])
@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_other_feature_counts(nfeat, reduce):
    """The reduction kernels' other instantiations (4 features in registers, any count through the generic path), with
    voxels on each side of the one-lane (8), one-wave (64) and workgroup thresholds."""
    rng = np.random.default_rng(20 + nfeat)
    parts = [_cell_point(rng, 30 + k, 40, 5, n) for k, n in enumerate((1, 2, 7, 8, 9, 33, 64, 65, 200))]
    pts = np.concatenate(parts)[rng.permutation(389)]
    pts = np.concatenate([pts, rng.uniform(-1, 1, (389, 2)).astype(np.float32)], 1)[:, :nfeat].copy()
    frames = [pts, pts[::-1].copy()]
    out = run_dyn(frames, RANGE, VSIZE, "zyx", reduce)
    ref = check_against_yardstick(out, frames, RANGE, VSIZE, "zyx", reduce)
    assert sorted(ref["counts"][:9].tolist()) == [1, 2, 7, 8, 9, 33, 64, 65, 200] and out["feat"].shape[1] == nfeat
