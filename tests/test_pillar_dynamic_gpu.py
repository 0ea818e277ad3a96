"""GPU suite: the dynamic pillar net (csrc/pillars_dyn.hip, models.DynamicPillarFeatureNet, PointPillars on the dynamic
voxelizer) against the golden recorded from the reference's own classes, the float64 restatement
(tests/pillar_dynamic_numpy.py), and -- bit for bit -- the hard kernel (csrc/pillars.hip) wherever no cap binds.

Accuracy: e = |got - ref| / absum, absum the abs chain of the winning point's sums; 1.5e-6 against float64 and 3e-6
against each recorded reference output, the bounds tests/test_pointpillars_golden_gpu.py holds the hard kernel to."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pillar_dynamic_numpy as RD
import pillars_fp64 as R
from test_pillar_dynamic_cpu import CONFIG, TAGS, golden
from test_pointpillars_golden import golden_geom, golden_layers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GEOM = dict(voxel_size=[0.2, 0.2, 8], pc_range=[-51.2, -51.2, -5, 51.2, 51.2, 3])


def _reader(filters, with_distance=False, seed=3, F=5, kind="DynamicPillarFeatureNet"):
    from al3d import synthetic
    from al3d.models import build_reader
    mod = build_reader(dict(type=kind, num_input_features=F, num_filters=filters, with_distance=with_distance, **GEOM))
    synthetic.seeded_init_(mod, seed=seed)
    return mod.cuda().eval()


def _layers(mod):
    out = []
    for p in mod.pfn_layers:
        bn = p.norm
        s, b = R.fold_bn(bn.weight.detach().cpu().numpy(), bn.bias.detach().cpu().numpy(),
                         bn.running_mean.cpu().numpy(), bn.running_var.cpu().numpy(), bn.eps)
        out.append((p.linear.weight.detach().cpu().numpy(), s, b))
    return out


def _geom(mod):
    return mod.vx, mod.vy, mod.x_offset, mod.y_offset, mod._with_distance


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.int32)


def _err(got, ref, absum):
    return float((np.abs(got.astype(np.float64) - ref) / absum).max()) if ref.size else 0.0


def _flatten(vox, n):
    """Slots -> (points [N,F] in pillar order, point2voxel [N], mean [M,F] f32): the mean as the voxelizer states it, the f32
    sum in ascending point index divided by (float)count (pillars.hip:81-82 forms it the same way)."""
    M, P, F = vox.shape
    n = np.minimum(np.asarray(n, np.int64), P)
    pts = np.concatenate([vox[i, :n[i]] for i in range(M)]) if M else np.zeros((0, F), np.float32)
    p2v = np.repeat(np.arange(M, dtype=np.int32), n)
    s = np.zeros((M, F), np.float32)
    for p in range(P):
        live = p < n
        s[live] = s[live] + vox[live, p]
    return pts.astype(np.float32), p2v, s / np.maximum(n, 1).astype(np.float32)[:, None]


def _net(mod):
    return mod.net(torch.device(DEV))


# ------------------------------------------------------------------------------------------------- 1. reference golden
@pytest.mark.parametrize("tag", TAGS)
def test_reader_matches_the_reference_pillar_nets(tag):
    """The golden's shuffled points through the real DynamicVoxelizer and the reader; rows matched by coordinate."""
    from al3d import detector_ops as D
    from al3d.models import build_reader
    g = golden()
    layers = golden_layers(g, tag)
    vs, pr = [float(v) for v in g["voxel_size"]], [float(v) for v in g["pc_range"]]
    r = build_reader(dict(type="DynamicPillarFeatureNet", num_input_features=5, num_filters=[64] * len(layers),
                          with_distance=tag.endswith("d1"), voxel_size=vs, pc_range=pr))
    r.load_state_dict({k: torch.from_numpy(g[f"{tag}.{k}"]) for k in r.state_dict()
                       if not k.endswith("num_batches_tracked")}, strict=False)
    r = r.to(DEV).eval()
    vox = D.DynamicVoxelizer(pr, vs, reduce="mean", order="zyx", device=DEV)
    pts, off = _dev(g["points"], g["point_offsets"])
    v = vox(pts, off)
    with torch.no_grad():
        got = r(pts, v["point2voxel"], v["feat"], v["coords"]).cpu().numpy()
    row = {tuple(c): i for i, c in enumerate(v["coords"].cpu().numpy().tolist())}
    assert len(row) == len(g["coords"]) == got.shape[0]
    got = got[[row[tuple(c)] for c in g["coords"].tolist()]]
    p2v, coords, _ = RD.voxelize(g["points"], g["point_offsets"], g["pc_range"], g["voxel_size"], g["grid"])
    ref, absum = RD.pfn_dynamic(g["points"], p2v, coords, layers, *golden_geom(g, tag))
    e = _err(got, ref, absum)
    print(f"{tag}: e = {e:.3e} against float64")
    assert e <= 1.5e-6, f"{tag}: e = {e:.3e} against float64"
    for which in ("out_det3d", "out_bevfusion"):
        e = _err(got, g[f"{tag}.{which}"].astype(np.float64), absum)
        print(f"{tag} {which}: e = {e:.3e}")
        assert e <= 3e-6, f"{tag} {which}: e = {e:.3e}"


# --------------------------------------------------------------------------------- 2. bit identities against the hard kernel
def _hard_case(seed, full):
    rng = np.random.default_rng(seed)
    P, M = 8, 500
    counts = np.full(M, P) if full else rng.integers(1, P + 1, size=M)
    vox, n, coords = R.make_case(rng, M, P, grid=(48, 40), batch=3, counts=counts)
    return vox, n, coords


@pytest.mark.parametrize("with_distance", [False, True])
def test_one_layer_bits_against_the_hard_kernel(with_distance):
    """Same points, same order, caps that do not bind: full rows are bit-equal; a row with n < P has
    hard == max(dynamic, relu(shift1)), the padded-slot floor being the one deliberate difference."""
    vox, n, coords = _hard_case(31, full=False)
    assert (n == 8).any() and (n < 8).any()
    mod = _reader([64], with_distance)
    hard = _net(mod).rows(*_dev(vox, n, coords))
    pts, p2v, mean = _flatten(vox, n)
    dyn = _net(mod).rows_dynamic(*_dev(pts, p2v, mean, coords))
    full = torch.from_numpy(n == 8).cuda()
    assert torch.equal(hard[full].view(torch.int32), dyn[full].view(torch.int32))
    floor = torch.relu(_net(mod).packs[0][2])[None]
    part = ~full
    assert torch.equal(hard[part].view(torch.int32), torch.maximum(dyn[part], floor).view(torch.int32))
    assert (dyn[part] < hard[part]).any()                            # the floor does bind somewhere


@pytest.mark.parametrize("filters,with_distance", [([64, 64], False), ([64, 64], True), ([256, 32], False)])
def test_two_layer_bits_against_the_hard_kernel(filters, with_distance):
    vox, n, coords = _hard_case(32, full=True)
    mod = _reader(filters, with_distance)
    hard = _net(mod).rows(*_dev(vox, n, coords))
    pts, p2v, mean = _flatten(vox, n)
    dyn = _net(mod).rows_dynamic(*_dev(pts, p2v, mean, coords))
    assert torch.equal(hard.view(torch.int32), dyn.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- 3. canvas
@pytest.mark.parametrize("filters", [[64], [64, 64]])
def test_canvas_equals_rows_plus_scatter(filters):
    from al3d import detector_ops as D
    vox, n, coords = _hard_case(33, full=False)
    B, ny, nx = 3, 40, 48
    coords = coords.copy()
    coords[7, 0] = B                       # outside the canvas: frame, row, column
    coords[8, 2] = ny
    coords[9, 3] = -1
    pts, p2v, mean = _flatten(vox, n)
    d = _dev(pts, p2v, mean, coords)
    net = _net(_reader(filters, True))
    a = net.canvas_dynamic(*d, B, ny, nx)
    b = net.canvas_dynamic(*d, B, ny, nx)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    rows = net.rows_dynamic(*d)
    split = D.pillar_scatter(rows, d[3], B, ny, nx)
    assert torch.equal(split.view(torch.int32), a.view(torch.int32))
    inside = np.ones(len(coords), bool)
    inside[7:10] = False
    hole = np.ones((B, ny, nx), bool)
    c = coords[inside]
    hole[c[:, 0], c[:, 2], c[:, 3]] = False
    an = a.cpu().numpy()
    assert (an[hole].view(np.int32) == 0).all()                      # +0.0 exactly, the dropped pillars included
    assert np.array_equal(_bits(an[c[:, 0], c[:, 2], c[:, 3]]), _bits(rows)[inside])
    assert an[~hole].any()


# ----------------------------------------------------------------------------------------------------------- 4. order
@pytest.mark.parametrize("filters", [[64], [64, 64]])
def test_point_order_and_launch_shape_leave_every_bit(filters):
    vox, n, coords = _hard_case(34, full=False)
    pts, p2v, mean = _flatten(vox, n)
    net = _net(_reader(filters, False))
    base = net.rows_dynamic(*_dev(pts, p2v, mean, coords))
    rng = np.random.default_rng(4)
    for k in range(3):
        perm = rng.permutation(len(pts))
        got = net.rows_dynamic(*_dev(pts[perm], p2v[perm], mean, coords))
        assert torch.equal(got.view(torch.int32), base.view(torch.int32)), k
    perm = rng.permutation(len(pts))
    for chunk, blocks in ((1, 0), (7, 3), (64, 1), (100000, 0), (3, 5)):
        for a, b in ((pts, p2v), (pts[perm], p2v[perm])):
            got = net.rows_dynamic(*_dev(a, b, mean, coords), chunk_points=chunk, max_blocks=blocks)
            assert torch.equal(got.view(torch.int32), base.view(torch.int32)), (chunk, blocks)


# ----------------------------------------------------------------------------------------------------------- 5. edges
def _cloud(rng, counts, F=5, grid=(48, 40), batch=2):
    """Pillars of the given point counts: (points, point2voxel, mean, coords), the points in pillar order."""
    M = len(counts)
    nx, ny = grid
    cells = rng.choice(batch * ny * nx, size=M, replace=False)
    b, rem = np.divmod(cells, ny * nx)
    y, x = np.divmod(rem, nx)
    coords = np.stack([b, np.zeros_like(b), y, x], 1).astype(np.int32)
    p2v = np.repeat(np.arange(M, dtype=np.int32), counts)
    N = len(p2v)
    pts = rng.normal(0, 1, size=(N, F))
    pts[:, 0] = (x[p2v] + rng.uniform(0, 1, N)) * 0.2 - 51.2
    pts[:, 1] = (y[p2v] + rng.uniform(0, 1, N)) * 0.2 - 51.2
    pts[:, 2] = rng.uniform(-5, 3, N)
    pts = pts.astype(np.float32)
    mean = np.zeros((M, F), np.float32)
    for i in range(N):                                   # ascending point index, f32 adds
        mean[p2v[i]] += pts[i]
    return pts, p2v, mean / np.maximum(np.asarray(counts), 1).astype(np.float32)[:, None], coords


def _check_fp64(mod, pts, p2v, mean, coords, **shape):
    got = _net(mod).rows_dynamic(*_dev(pts, p2v, mean, coords), **shape)
    ref, absum = RD.pfn_dynamic(pts, p2v, coords, _layers(mod), *_geom(mod), mean=mean)
    e = _err(got.cpu().numpy(), ref, absum)
    assert got.shape == ref.shape and e <= 1.5e-6, f"e = {e:.3e}"
    return got


def test_empty_inputs():
    mod = _reader([64, 64])
    net = _net(mod)
    rng = np.random.default_rng(50)
    pts, p2v, mean, coords = _cloud(rng, [3, 1, 2])
    none = net.rows_dynamic(*_dev(pts[:0], p2v[:0], mean, coords))              # npts = 0
    assert tuple(none.shape) == (3, 64) and (_bits(none) == 0).all()
    c = net.canvas_dynamic(*_dev(pts[:0], p2v[:0], mean, coords), 2, 40, 48)
    assert tuple(c.shape) == (2, 40, 48, 64) and (_bits(c) == 0).all()
    rows = net.rows_dynamic(*_dev(pts, np.full_like(p2v, -1), mean[:0], coords[:0]))   # M = 0: every point unassigned
    assert tuple(rows.shape) == (0, 64)
    c = net.canvas_dynamic(*_dev(pts, np.full_like(p2v, -1), mean[:0], coords[:0]), 2, 40, 48)
    assert (_bits(c) == 0).all()
    skipped = net.rows_dynamic(*_dev(pts, np.full_like(p2v, -1), mean, coords))   # every point2voxel = -1
    assert (_bits(skipped) == 0).all()
    for m in (_reader([64]), mod):                                                # one pillar of one point
        pts1, p2v1, mean1, coords1 = _cloud(rng, [1])
        _check_fp64(m, pts1, p2v1, mean1, coords1)


@pytest.mark.parametrize("filters", [[64], [64, 64]])
def test_one_pillar_of_5000_points_among_300_singletons(filters):
    """The long run crosses every chunk boundary of the launch (64-point chunks by default), in pillar order and shuffled;
    point counts of a whole number of chunks, and one point more and less."""
    rng = np.random.default_rng(51)
    mod = _reader(filters)
    for big in (5000, 64 * 78 - 300 - 1, 64 * 78 - 300, 64 * 78 - 300 + 1):
        counts = np.ones(301, np.int64)
        counts[150] = big
        pts, p2v, mean, coords = _cloud(rng, counts)
        got = _check_fp64(mod, pts, p2v, mean, coords)
        perm = rng.permutation(len(pts))
        again = _net(mod).rows_dynamic(*_dev(pts[perm], p2v[perm], mean, coords))
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        for chunk in (63, 65):
            again = _net(mod).rows_dynamic(*_dev(pts, p2v, mean, coords), chunk_points=chunk)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("npts", [1, 63, 65, 257])
def test_point_counts_around_the_wave_and_block_sizes(npts):
    rng = np.random.default_rng(52 + npts)
    counts = np.bincount(rng.integers(0, max(1, npts // 3), size=npts))
    counts = counts[counts > 0]
    pts, p2v, mean, coords = _cloud(rng, counts)
    perm = rng.permutation(npts)
    for filters in ([64], [64, 64]):
        mod = _reader(filters)
        a = _check_fp64(mod, pts, p2v, mean, coords)
        b = _check_fp64(mod, pts[perm], p2v[perm], mean, coords)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("F", [3, 5, 10])
@pytest.mark.parametrize("U1", [16, 64, 128])
@pytest.mark.parametrize("U2", [0, 16, 64])
@pytest.mark.parametrize("with_distance", [False, True])
def test_sizes(F, U1, U2, with_distance):
    """F, U1, U2 (0: one layer) and with_distance over their ranges: float64, and the hard kernel's bits on full pillars."""
    rng = np.random.default_rng(F * 1000 + U1 * 3 + U2 + int(with_distance))
    filters = [2 * U1, U2] if U2 else [U1]
    mod = _reader(filters, with_distance, F=F)
    counts = rng.integers(1, 40, size=90)
    pts, p2v, mean, coords = _cloud(rng, counts, F=F)
    perm = rng.permutation(len(pts))
    _check_fp64(mod, pts[perm], p2v[perm], mean, coords)
    vox, n, c = R.make_case(rng, 70, 6, F=F, grid=(48, 40), batch=2, counts=np.full(70, 6))
    hard = _net(mod).rows(*_dev(vox, n, c))
    dyn = _net(mod).rows_dynamic(*_dev(*_flatten(vox, n), c))
    assert torch.equal(hard.view(torch.int32), dyn.view(torch.int32))


def test_all_negative_pillar_is_plus_zero():
    """Layer 1 reads the intensity column alone, scale 1, shift 0: a pillar whose intensities are negative or -0.0 has
    only negative (or -0.0) pre-activations; its row is +0.0 by bit pattern."""
    mod = _reader([64])
    with torch.no_grad():
        p = mod.pfn_layers[0]
        p.linear.weight.zero_()
        p.linear.weight[:, 3] = torch.linspace(0.5, 2.0, 64, device=DEV)
        p.norm.weight.fill_(1.0)
        p.norm.bias.zero_()
        p.norm.running_mean.zero_()
        p.norm.running_var.fill_(1.0 - p.norm.eps)
    rng = np.random.default_rng(53)
    pts, p2v, mean, coords = _cloud(rng, [9, 6, 70, 1])
    pts[:, 3] = np.abs(pts[:, 3]) + 0.1
    sel = np.flatnonzero(p2v == 2)
    pts[sel, 3] = -np.abs(pts[sel, 3])
    pts[sel[::3], 3] = -0.0
    perm = rng.permutation(len(pts))
    for a, b in ((pts, p2v), (pts[perm], p2v[perm])):
        got = _net(mod).rows_dynamic(*_dev(a, b, mean, coords))
        bits = _bits(got)
        assert (bits[2] == 0).all()
        assert (got[[0, 1, 3]] > 0).all()


@pytest.mark.parametrize("filters", [[64], [64, 64]])
def test_nan_feature_equals_the_hard_kernel(filters):
    """A NaN intensity (that point's pre-activations are NaN and contribute 0) and a NaN x (the pillar's mean is NaN, the
    whole pillar contributes 0): the hard kernel's bits on the same slots."""
    vox, n, coords = _hard_case(35, full=True)
    vox[0, 2, 3] = np.nan
    vox[1, 0, 0] = np.nan
    mod = _reader(filters, True)
    hard = _net(mod).rows(*_dev(vox, n, coords))
    pts, p2v, mean = _flatten(vox, n)
    assert np.isnan(mean[1, 0]) and not np.isnan(mean[0, :3]).any()
    dyn = _net(mod).rows_dynamic(*_dev(pts, p2v, mean, coords))
    assert torch.equal(hard.view(torch.int32), dyn.view(torch.int32))
    assert torch.isfinite(dyn).all() and dyn[0].any()
    if len(filters) == 1:
        assert (_bits(dyn[1]) == 0).all()


def test_point2voxel_out_of_range_sets_the_status_bit():
    from al3d import lib
    rng = np.random.default_rng(54)
    pts, p2v, mean, coords = _cloud(rng, rng.integers(1, 9, size=60))
    M = len(coords)
    mod = _reader([64, 64])
    net = _net(mod)
    skip = p2v.copy()
    skip[100] = -1
    want = net.rows_dynamic(*_dev(pts, skip, mean, coords))
    assert int(net._status.item()) == 0
    for bad_value in (M, -2, 2 ** 31 - 1):
        bad = p2v.copy()
        bad[100] = bad_value
        got = net.rows_dynamic(*_dev(pts, bad, mean, coords), check=False)
        assert int(net._status.item()) & 1
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))       # the point is skipped, nothing else moves
        with pytest.raises(lib.Al3dError, match="point2voxel"):
            net.dynamic_status()
        assert int(net._status.item()) == 0
    with pytest.raises(lib.Al3dError, match="point2voxel"):
        net.rows_dynamic(*_dev(pts, bad, mean, coords))


# ------------------------------------------------------------------------------------------------------ 6. one full frame
def test_full_frame_300000_points():
    """300,000 seeded points on the config's 512 x 512 grid through the real voxelizer, two layers of 64."""
    from al3d import detector_ops as D
    rng = np.random.default_rng(60)
    N = 300_000
    pts = np.zeros((N, 5), np.float32)
    near = rng.random(N) < 0.4                           # a dense near range: pillars of hundreds of points
    pts[:, :2] = np.where(near[:, None], rng.normal(0, 2.0, (N, 2)), rng.uniform(-51.2, 51.2, (N, 2)))
    pts[:, 2] = rng.uniform(-5, 3, N)
    pts[:, 3] = rng.uniform(0, 1, N)
    pts[:, 4] = rng.uniform(0, 0.5, N)
    pts[:10, 0] = 60.0                                   # out of range: point2voxel -1
    mod = _reader([64, 64])
    vox = D.DynamicVoxelizer(GEOM["pc_range"], GEOM["voxel_size"], reduce="mean", order="zyx", device=DEV)
    p, off = _dev(pts, np.array([0, N], np.int64))
    v = vox(p, off)
    got = mod(p, v["point2voxel"], v["feat"], v["coords"]).cpu().numpy()
    p2v, coords = v["point2voxel"].cpu().numpy(), v["coords"].cpu().numpy()
    assert (p2v[:10] == -1).all() and int(v["num_points"].max()) >= 100
    ref, absum = RD.pfn_dynamic(pts, p2v, coords, _layers(mod), *_geom(mod))
    e = _err(got, ref, absum)
    print(f"full frame: {len(coords)} pillars, largest {int(v['num_points'].max())} points, e = {e:.3e}")
    assert e <= 1.5e-6, f"e = {e:.3e}"
    canvas = _net(mod).canvas_dynamic(p, v["point2voxel"], v["feat"], v["coords"], 1, 512, 512).cpu().numpy()
    assert np.array_equal(_bits(canvas[coords[:, 0], coords[:, 2], coords[:, 3]]), _bits(got))
    assert np.count_nonzero(canvas.any(-1)) <= len(coords)


def test_pointpillars_graph_on_the_device_loader():
    """PointPillars with the dynamic reader over DeviceSweepLoader(keep_points=True) batches of a two-frame synthetic pool:
    the embedding is the same bits twice, and equals reader, scatter and neck run module by module."""
    from al3d import detector_ops as D
    from al3d import synthetic
    from al3d.datasets import DeviceSweepLoader, PoolFrames
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(CONFIG)
    m = build_detector(dict(
        type="PointPillars", reader=dict(cfg.model.reader), backbone=dict(cfg.model.backbone),
        neck=dict(type="RPN", layer_nums=[1, 1], ds_layer_strides=[2, 2], ds_num_filters=[64, 128],
                  us_layer_strides=[1, 2], us_num_filters=[64, 64], num_input_features=64),
        bbox_head=None))
    synthetic.seeded_init_(m, seed=0)
    m = m.cuda().eval()
    pool = PoolFrames.from_synthetic(2, torch.device(DEV), seed=7)
    loader = DeviceSweepLoader(pool, cfg.voxel_generator, None, batch_size=2, device=DEV, keep_points=True)
    ex = next(iter(loader))
    assert ex["point2voxel"].shape[0] == ex["points"].shape[0] and "voxels" not in ex
    assert m.prepare(ex) is None
    with torch.no_grad():
        embs = []
        for _ in range(2):
            preds, middle = m(ex, return_loss=False, estimate=True)
            embs.append(middle[-1].mean(-1).mean(-1).clone())
        nx, ny = int(ex["shape"][0][0]), int(ex["shape"][0][1])
        rows = m.reader(ex["points"], ex["point2voxel"], ex["voxel_features"], ex["coordinates"])
        canvas = m.backbone(rows, ex["coordinates"], 2, [nx, ny, 1])
        y = m.neck(canvas)
        emb2 = m.neck.embedding if m.neck.embedding is not None else D.gap_nhwc(y)
    assert tuple(embs[0].shape) == (2, 128) and torch.isfinite(embs[0]).all() and len(preds) == 2
    assert torch.equal(embs[0].view(torch.int32), embs[1].view(torch.int32))
    assert torch.equal(embs[0].view(torch.int32), emb2.view(torch.int32))
    # without the points the detector says what the loader needs
    bare = next(iter(DeviceSweepLoader(pool, cfg.voxel_generator, None, batch_size=2, device=DEV)))
    with pytest.raises(RuntimeError, match="keep_points=True"):
        m(bare, return_loss=False, estimate=True)


# -------------------------------------------------------------------------------------------------------------- 7. CLI
def test_cli_dynamic_pointpillars_config(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "active_select.py"), "--config", CONFIG, "--budget", "20", "--pred",
           "--synthetic-scenes", "1", "--batch", "8"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for _ in range(2):                       # bootstrap the empty buffer, then sweep + select
        r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    out = json.load(open(tmp_path / "data" / "buffers" / "bevfusion_pointpillars_dynamic_stf.json"))
    assert list(out) == ["0", "20"] and len(out["20"]) >= 1 and len(set(out["20"])) == len(out["20"])
