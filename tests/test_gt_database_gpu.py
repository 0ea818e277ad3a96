"""GPU suite of the ground-truth database builder (csrc/points_in_boxes.hip, selector_ops.points_in_boxes*, al3d.ops.
points_in_rbbox, al3d.datasets.create_groundtruth_database).

Everything is compared exactly.  The membership rule is float32 arithmetic in a fixed order with no fused multiply-add,
so the kernels owe the reference's masks bit for bit (tests/golden/gt_database.npz: the reference's own
``points_in_rbbox`` and ``create_groundtruth_database``), and at the sizes the golden does not have they owe the numpy
yardstick of tests/gt_database_numpy.py, which tests/test_gt_database_cpu.py pins to the same golden."""
import os
import pickle

import numpy as np
import pytest
import torch

import gt_database_numpy as Y

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOTS = 32 * 4                                               # AL3D_PIB_GROUPS x waves of AL3D_PIB_THREADS: one wave's chunk is 64 points


def _t(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _batch(frames):
    """[(points [P, F], planes [n, 6, 4], centres [n, 3])] -> the arrays of one call."""
    F = frames[0][0].shape[1]
    points = np.concatenate([f[0] for f in frames]).astype(np.float32).reshape(-1, F)
    planes = np.concatenate([f[1] for f in frames]).astype(np.float32).reshape(-1, 6, 4)
    centres = np.concatenate([f[2] for f in frames]).astype(np.float32).reshape(-1, 3)
    point_off = np.cumsum([0] + [len(f[0]) for f in frames]).astype(np.int64)
    box_off = np.cumsum([0] + [len(f[1]) for f in frames]).astype(np.int32)
    return points, point_off, planes, centres, box_off


def _golden_batch():
    g = Y.golden()
    return _batch([(g[f"{b}_points"], g[f"{b}_planes"], g[f"{b}_boxes"][:, :3]) for b in ("f0", "f1", "f2", "edge")])


def _run(batch, nf, launch=None):
    """selector_ops.points_in_boxes on the batch's own planes -> numpy (rows, index, counts, offsets)."""
    from al3d import selector_ops as ops
    points, point_off, planes, centres, box_off = batch
    boxes = np.concatenate([centres, np.zeros((len(centres), 4), np.float32)], axis=1)     # only the centres are read
    out = ops.points_in_boxes(_t(points), _t(point_off), boxes, _t(box_off), nf, planes=_t(planes), launch=launch)
    return tuple(o.cpu().numpy() for o in out)


def _rows_equal(a, b):
    """Bit for bit -- except that a NaN only has to be a NaN: the edge block subtracts NaN centres from NaN points, and
    IEEE 754 leaves the sign and payload of a NaN that arithmetic produces to the implementation (the host's and the
    device's differ).  Finite values, infinities and zeros compare by their bits."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan])


def _assert_same(got, want, what=""):
    for a, b, name in zip(got, want, ("rows", "index", "counts", "offsets")):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        assert _rows_equal(a, b) if name == "rows" else a.tobytes() == b.tobytes(), (what, name)


_yard = {}


def _golden_yardstick(nf):
    if nf not in _yard:
        points, point_off, planes, centres, box_off = _golden_batch()
        with np.errstate(invalid="ignore"):
            _yard[nf] = Y.compact(points, point_off, planes, centres, box_off, nf)
    return _yard[nf]


@pytest.mark.parametrize("block", ("f0", "f1", "f2", "edge"))
def test_mask_kernel_equals_the_reference_mask(block):
    from al3d import selector_ops as ops
    g = Y.golden()
    m = ops.points_in_boxes_mask(_t(g[f"{block}_points"]), _t(g[f"{block}_planes"]))
    assert m.dtype == torch.uint8 and tuple(m.shape) == g[f"{block}_mask"].shape
    assert np.array_equal(m.cpu().numpy().astype(bool), g[f"{block}_mask"])
    for launch in ((64, 1), (128, 7), (256, 63), (64, 64)):
        again = ops.points_in_boxes_mask(_t(g[f"{block}_points"]), _t(g[f"{block}_planes"]), launch=launch)
        assert torch.equal(again, m), launch


@pytest.mark.parametrize("block", ("f0", "f1", "f2", "edge"))
def test_points_in_rbbox_equals_the_reference(block):
    import al3d.ops
    g = Y.golden()
    with np.errstate(invalid="ignore"):
        m = al3d.ops.points_in_rbbox(g[f"{block}_points"], g[f"{block}_boxes"])
    assert m.dtype == np.bool_ and np.array_equal(m, g[f"{block}_mask"])


@pytest.mark.parametrize("nf", (5, 3))
def test_count_and_gather_on_the_golden_equal_the_yardstick_bits(nf):
    g = Y.golden()
    want = _golden_yardstick(nf)
    got = _run(_golden_batch(), nf)
    _assert_same(got, want)
    # ... and the reference directly: the counts are its masks' column sums, the rows its files
    masks = [g[f"{b}_mask"] for b in ("f0", "f1", "f2", "edge")]
    assert np.array_equal(got[2], np.concatenate([m.sum(0) for m in masks]).astype(np.int32))
    if nf == 5:
        files = Y.golden_files(g)
        r = 0
        for f in range(3):
            for i, name in enumerate(g[f"f{f}_gt_names"]):
                rows = got[0][got[3][r]:got[3][r + 1]]
                assert rows.tobytes() == files[f"{f}_{name}_{i}.bin"].tobytes(), (f, i)
                r += 1


def _random_frame(rng, n_points, n_boxes, F=5):
    from al3d.detector_ops import box_planes
    pts = rng.uniform(-10, 10, (n_points, F)).astype(np.float32)
    boxes = np.concatenate([rng.uniform(-8, 8, (n_boxes, 3)), rng.uniform(2, 16, (n_boxes, 3)), rng.normal(0, 1, (n_boxes, 2)),
                            rng.uniform(-3.2, 3.2, (n_boxes, 1))], axis=1).astype(np.float32)
    return pts, box_planes(boxes), boxes[:, :3]


# (points, boxes) per frame: no points, no boxes, both; 1 / 64 / 65 / 130 boxes against 1 / 63 / 64 / 65 points; a frame of
# one point per wave slot's chunk of 64 points, +- 1 (where the spans go from one chunk to two)
SIZE_FRAMES = [(0, 3), (5, 0), (0, 0), (1, 1), (63, 64), (64, 65), (65, 130), (64 * SLOTS - 1, 2), (64 * SLOTS, 3),
               (64 * SLOTS + 1, 1), (2 * 64 * SLOTS + 1, 2)]


@pytest.fixture(scope="module")
def size_case():
    rng = np.random.default_rng(7)
    batch = _batch([_random_frame(rng, p, b) for p, b in SIZE_FRAMES])
    want = Y.compact(batch[0], batch[1], batch[2], batch[3], batch[4], 5)
    assert want[2].max() > 64 and (want[2] == 0).any()       # boxes with more members than a wave, and empty ones
    return batch, want


def test_size_edges_equal_the_yardstick(size_case):
    batch, want = size_case
    _assert_same(_run(batch, 5), want)
    points, point_off, planes, centres, box_off = batch
    for b in range(len(SIZE_FRAMES)):                        # every frame alone: the same rows, re-based
        one = (points[point_off[b]:point_off[b + 1]], np.array([0, point_off[b + 1] - point_off[b]], np.int64),
               planes[box_off[b]:box_off[b + 1]], centres[box_off[b]:box_off[b + 1]],
               np.array([0, box_off[b + 1] - box_off[b]], np.int32))
        rows, index, counts, offsets = _run(one, 5)
        r0, r1 = box_off[b], box_off[b + 1]
        lo, hi = want[3][r0], want[3][r1]
        assert np.array_equal(counts, want[2][r0:r1]), SIZE_FRAMES[b]
        assert rows.tobytes() == want[0][lo:hi].tobytes() and np.array_equal(index + point_off[b], want[1][lo:hi]), SIZE_FRAMES[b]


LAUNCHES = [(1, 64, 64), (1, 256, 1), (3, 128, 7), (32, 64, 63), (64, 256, 64), (1024, 64, 5), (5, 256, 33)]


@pytest.mark.parametrize("launch", LAUNCHES)
def test_every_launch_shape_gives_the_default_bytes(size_case, launch):
    batch, want = size_case
    _assert_same(_run(batch, 5, launch), want, launch)
    _assert_same(_run(_golden_batch(), 5, launch), _golden_yardstick(5), launch)


def test_two_runs_are_identical():
    a, b = _run(_golden_batch(), 5), _run(_golden_batch(), 5)
    _assert_same(a, b)


def _low_level(points, point_off, planes, box_off):
    from al3d import selector_ops as ops
    counts, ws, status = ops.points_in_boxes_count(_t(points), _t(point_off), _t(planes), _t(box_off))
    return counts, ws, status


def test_bad_offsets_set_the_status_and_write_nothing():
    from al3d import lib, selector_ops as ops
    g = Y.golden()
    points, planes, centres = g["f2_points"], g["f2_planes"], g["f2_boxes"][:, :3]
    P, R = len(points), len(planes)
    good = Y.mask(points, planes[:10]).sum(0).astype(np.int32)
    cases = [(np.array([0, 10, 4], np.int32), np.array([0, P, P], np.int64), ops.PIB_BAD_BOX_OFF),       # descending
             (np.array([0, 10, R + 1], np.int32), np.array([0, P, P], np.int64), ops.PIB_BAD_BOX_OFF),   # past the end
             (np.array([0, 10, R], np.int32), np.array([0, P, P + 1], np.int64), ops.PIB_BAD_POINT_OFF)]
    for box_off, point_off, bit in cases:
        counts, ws, status = _low_level(points, point_off, planes, box_off)
        assert int(status.item()) == bit
        counts = counts.cpu().numpy()
        assert np.array_equal(counts[:10], good) and not counts[10:].any()      # the good frame is counted, the bad one is empty
        off = np.zeros(R + 1, np.int64)
        np.cumsum(counts, out=off[1:])
        T = int(off[-1])
        from al3d.selector_ops import _ptr, _stream
        rows = torch.full((T + 8, 5), -7.0, device=DEV)
        index = torch.full((T + 8,), -7, dtype=torch.int64, device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        d = [_t(points), _t(point_off), _t(planes), _t(box_off), _t(off), _t(centres)]
        lib.call("al3d_points_in_boxes_gather_f32", _ptr(d[0]), P, 5, _ptr(d[1]), 2, _ptr(d[2]), _ptr(d[3]), R, _ptr(d[4]),
                 _ptr(d[5]), _ptr(ws), _ptr(rows), 5, _ptr(index), T + 8, _ptr(st), _stream())
        assert int(st.item()) == bit
        assert bool((rows[T:] == -7.0).all()) and bool((index[T:] == -7).all())  # nothing past the good frame's rows
        want = Y.compact(points, point_off[:2], planes[:10], centres[:10], box_off[:2], 5)
        assert rows[:T].cpu().numpy().tobytes() == want[0].tobytes()
        with pytest.raises(lib.Al3dError):
            ops.points_in_boxes(_t(points), _t(point_off), g["f2_boxes"], _t(box_off), 5)
    # every frame bad: no count, no row
    counts, ws, status = _low_level(points, np.array([0, P], np.int64), planes, np.array([R, 0], np.int32))
    assert int(status.item()) == ops.PIB_BAD_BOX_OFF and not counts.cpu().numpy().any()


def test_gather_refuses_the_workspace_of_another_launch_shape():
    from al3d import selector_ops as ops
    points, point_off, planes, centres, box_off = _golden_batch()
    d = dict(points=_t(points), point_off=_t(point_off), planes=_t(planes), box_off=_t(box_off))
    counts, ws, _ = ops.points_in_boxes_count(**d, launch=(32, 256, 64))
    off = torch.zeros(len(planes) + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(counts, 0, out=off[1:])
    big = torch.empty(int(ws.numel()) * 4, dtype=torch.uint8, device=DEV)
    big[:ws.numel()] = ws
    rows, index, st = ops.points_in_boxes_gather(d["points"], d["point_off"], d["planes"], d["box_off"], off, _t(centres), big,
                                                 int(off[-1]), 5, launch=(64, 256, 64))
    assert int(st.item()) == ops.PIB_BAD_WORKSPACE
    rows, index, st = ops.points_in_boxes_gather(d["points"], d["point_off"], d["planes"], d["box_off"], off, _t(centres), ws,
                                                 int(off[-1]), 5, launch=(32, 256, 9))         # the tile is free
    assert int(st.item()) == 0 and _rows_equal(rows.cpu().numpy(), _golden_yardstick(5)[0])


def test_mask_past_2_31_bytes():
    """[P, R] with P * R > 2^31: the row offsets are 64-bit."""
    from al3d import selector_ops as ops
    rng = np.random.default_rng(3)
    P, R = 33000, 66000
    assert P * R > 2 ** 31
    pts, planes, _ = _random_frame(rng, P, 64)
    planes = np.tile(planes, (R // 64 + 1, 1, 1))[:R]
    m = ops.points_in_boxes_mask(_t(pts), _t(planes))
    for i in (0, 1, P // 2, P - 2, P - 1):
        assert np.array_equal(m[i].cpu().numpy().astype(bool), Y.mask(pts[i:i + 1], planes)[0]), i
    assert int(m[-1].sum()) > 0
    del m
    torch.cuda.empty_cache()


def _tree(root):
    out = {}
    for dp, _, fns in os.walk(root):
        for fn in fns:
            p = os.path.join(dp, fn)
            with open(p, "rb") as f:
                out[os.path.relpath(p, root)] = f.read()
    return out


def test_end_to_end_on_the_golden_pool(tmp_path):
    from al3d.datasets import create_groundtruth_database
    g = Y.golden()
    trees = []
    for run in ("a", "b"):
        root = tmp_path / run
        root.mkdir()
        info_path = Y.write_golden_pool(g, root)
        before = set(os.listdir(root))
        db = create_groundtruth_database("NUSC", str(root), info_path, nsweeps=int(g["nsweeps"]), suffix=str(g["suffix"]),
                                         batch_size=2)
        stem = f"gt_database_{int(g['nsweeps'])}sweeps_withvelo_{g['suffix']}"
        pkl = f"dbinfos_train_{int(g['nsweeps'])}sweeps_withvelo_{g['suffix']}.pkl"
        assert set(os.listdir(root)) - before == {stem, pkl}
        Y.assert_files(root / stem, g)
        with open(root / pkl, "rb") as f:
            loaded = pickle.load(f)
        Y.assert_dbinfos(loaded, g, "db")
        Y.assert_dbinfos(db, g, "db")
        trees.append({k: v for k, v in _tree(root).items() if k == pkl or k.startswith(stem)})
    assert trees[0].keys() == trees[1].keys() and all(trees[0][k] == trees[1][k] for k in trees[0])   # byte-identical runs
    # used_classes, relative_path=False, own paths, one frame a batch
    root = tmp_path / "a"
    create_groundtruth_database("NUSC", str(root), Y.write_golden_pool(g, root), used_classes=g["used_classes"].tolist(),
                                db_path=root / "alt_db", dbinfo_path=root / "alt.pkl", relative_path=False,
                                nsweeps=int(g["nsweeps"]), suffix=str(g["suffix"]), batch_size=1)
    Y.assert_files(root / "alt_db", g)
    with open(root / "alt.pkl", "rb") as f:
        Y.assert_dbinfos(pickle.load(f), g, "alt", root=root)


def test_loader_points_equal_the_reference_loader(tmp_path):
    """The points-only loader: the merged clouds of the golden pool, bit for bit, in list order."""
    from al3d.datasets import SweepPointsLoader
    g = Y.golden()
    with open(Y.write_golden_pool(g, tmp_path), "rb") as f:
        infos = pickle.load(f)
    loader = SweepPointsLoader(infos, batch_size=2, device=DEV, nsweeps=int(g["nsweeps"]))
    seen = []
    for points, off, ids in loader:
        off = off.cpu().numpy()
        for k, i in enumerate(ids):
            got = points[off[k]:off[k + 1]].cpu().numpy()
            assert got.tobytes() == g[f"f{i}_points"].tobytes(), i
            seen.append(i)
    assert seen == [0, 1, 2]
    loader.reader.close()
