"""GPU suite: the hard voxelizer (csrc/voxelize.hip) on the cases of tests/voxel_cases.py -- the cap inside a batch, every
gather shape, frame boundaries inside a wave, a first-index grid that an earlier call must have left clean, and the cell
arithmetic round every cell edge of the real geometries.  Everything is compared bit for bit, per frame, with the CPU
oracle; tests/test_voxel_cases_cpu.py shows what each case would catch."""
import numpy as np
import pytest
import torch

import voxel_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_EXPECTED = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def expected(oracle, case):
    """The oracle's per-frame results of a case, computed once."""
    if case["name"] not in _EXPECTED:
        g = case["geom"]
        _EXPECTED[case["name"]] = [oracle.voxelize(f, g["range"][:3], g["vsize"], g["grid"], case["max_points"],
                                                   case["max_voxels"]) for f in case["frames"]]
    return _EXPECTED[case["name"]]


def make_voxelizer(case, max_batch=None):
    from al3d import detector_ops as D
    g = case["geom"]
    vox = D.Voxelizer(g["range"], g["vsize"], case["max_points"], case["max_voxels"],
                      max_batch=max_batch or max(1, len(case["frames"])), device=DEV)
    assert vox.grid_size.tolist() == list(g["grid"])
    return vox


def device_input(case):
    parts = [f for f in case["frames"] if len(f)] + ([case["tail"]] if case["tail"] is not None else [])
    pts = np.concatenate(parts) if parts else np.zeros((0, case["nfeat"]), np.float32)
    off = np.concatenate([[0], np.cumsum([len(f) for f in case["frames"]])]).astype(np.int64)
    return torch.from_numpy(pts).to(DEV), torch.from_numpy(off).to(DEV)


def run(vox, case, want_voxels):
    pts, off = device_input(case)
    out = vox(pts, off, want_voxels=want_voxels)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def check(out, want, want_voxels):
    """One call's output against the per-frame oracle results: rows, counts, slots and means as bits, plus the frame
    bookkeeping."""
    m = [len(w[1]) for w in want]
    assert out["num_voxels"].tolist() == m
    assert out["row_base"].tolist() == np.concatenate([[0], np.cumsum(m)]).tolist()
    assert len(out["coords"]) == len(out["feat"]) == len(out["num_points"]) == sum(m)
    row = 0
    for b, (v, c, n, f) in enumerate(want):
        sl = slice(row, row + len(c))
        assert np.all(out["coords"][sl, 0] == b), b
        assert np.array_equal(out["coords"][sl, 1:], c), b
        assert np.array_equal(out["num_points"][sl], n), b
        assert np.array_equal(_bits(out["feat"][sl]), _bits(f)), b
        if want_voxels:
            assert np.array_equal(_bits(out["voxels"][sl]), _bits(v)), b
        row += len(c)
    if not want_voxels:
        assert out["voxels"] is None


def run_both_ways(oracle, case, vox=None):
    """With and without the padded point slots: each equals the oracle, and the two agree bit for bit."""
    vox = vox or make_voxelizer(case)
    want = expected(oracle, case)
    a, b = run(vox, case, True), run(vox, case, False)
    check(a, want, True)
    check(b, want, False)
    for k in ("feat", "coords", "num_points"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    return a


def test_cap_in_batch(oracle):
    case = V.cap_in_batch()
    out = run_both_ways(oracle, case)
    assert out["num_voxels"].tolist() == [50, 50, 0, 50, 49] and out["row_base"].tolist() == [0, 50, 100, 100, 150, 199]


@pytest.mark.parametrize("nfeat", V.GATHER_NFEAT)
@pytest.mark.parametrize("max_points", V.GATHER_MAX_POINTS)
def test_gather_sweep(oracle, max_points, nfeat):
    out = run_both_ways(oracle, V.gather_sweep(max_points, nfeat))
    assert out["num_points"].max() == max_points and out["voxels"].shape[1:] == (max_points, nfeat)


def test_frame_edges(oracle):
    case = V.frame_edges()
    out = run_both_ways(oracle, case)
    zyx = V.cell_coords_zyx([case["shared"]], case["geom"])[0]
    hits = np.flatnonzero(np.all(out["coords"][:, 1:] == zyx, axis=1))
    assert out["coords"][hits, 0].tolist() == [b for b, n in enumerate(V.LENGTHS) if n]     # one voxel in every frame


def test_empty_frames_at_the_ends_and_an_empty_batch(oracle):
    ends, none = V.empty_frame_cases()
    out = run_both_ways(oracle, ends)
    assert out["num_voxels"].tolist() == [0, 0, 3, 0]
    out = run_both_ways(oracle, none)
    assert out["num_voxels"].tolist() == [0, 0, 0] and out["row_base"].tolist() == [0, 0, 0, 0]
    assert out["feat"].shape == (0, 5) and out["coords"].shape == (0, 4)


@pytest.mark.parametrize("name", ["capped", "tail", "batch_sizes"])
def test_stale_grid(oracle, name):
    """One resident voxelizer sees the calls in turn; each later call must come out as on a fresh object (and as the
    oracle): its cells sit at larger indices than in the call before, so a cell left behind would lose its leader."""
    calls = dict(V.stale_grid_pairs())[name]
    resident = make_voxelizer(calls[0], max_batch=8)
    for i, case in enumerate(calls):
        got = run_both_ways(oracle, case, vox=resident)
        if i:
            fresh = run(make_voxelizer(case, max_batch=8), case, True)
            for k in ("feat", "coords", "num_points", "voxels", "num_voxels", "row_base"):
                assert np.array_equal(got[k].view(np.int32), fresh[k].view(np.int32)), (case["name"], k)


@pytest.mark.parametrize("name", sorted(V.GEOMETRIES))
def test_cell_arithmetic(oracle, name):
    """Coordinates -3..+3 ulps round every cell edge of the geometry, NaN / inf / 1e38 one coordinate at a time (and the
    zeros and denormals on KITTI's x = 0 edge): the oracle, numpy's float32 floor((p - min) / vs) with first-appearance
    order by np.unique, and the dynamic voxelizer (which shares vox_cell.h) as a sorted coordinate set."""
    from al3d import detector_ops as D
    case = V.cell_arithmetic(name)
    g = case["geom"]
    out = run_both_ways(oracle, case, vox=make_voxelizer(case, max_batch=1))
    order, _ = V.first_appearance(V.cells_of(case["frames"][0], g))
    assert np.array_equal(out["coords"][:, 1:], V.cell_coords_zyx(order, g)) and np.all(out["coords"][:, 0] == 0)
    dyn = D.DynamicVoxelizer(g["range"], g["vsize"], device=DEV)
    pts, off = device_input(case)
    d = dyn(pts, off, want_point_coords=True)
    assert np.array_equal(d["coords"].cpu().numpy(), np.unique(out["coords"], axis=0))
    pc = d["point_coords"].cpu().numpy()
    cells = V.cells_of(case["frames"][0], g)
    want_pc = np.where((cells >= 0)[:, None], V.cell_coords_zyx(np.maximum(cells, 0), g)[:, ::-1], -1)
    assert np.array_equal(pc, want_pc)
