"""CPU suite: the hard-voxelizer cases of tests/voxel_cases.py have teeth.  For every case the numpy restatement of the
contract equals the CPU oracle bit for bit, and a deliberately wrong restatement -- the mistake the case was built to
catch -- does not.  These are conditions on the cases, not measurements of the kernel (tests/test_voxel_edges_gpu.py runs
the HIP code on the same cases)."""
import ctypes

import numpy as np
import pytest

import voxel_cases as V


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def oracle_frames(oracle, case):
    g = case["geom"]
    return [oracle.voxelize(f, g["range"][:3], g["vsize"], g["grid"], case["max_points"], case["max_voxels"])
            for f in case["frames"]]


def same(a, b):
    """(voxels, coords, num_points, feat) tuples equal bit for bit."""
    return (a[1].shape == b[1].shape and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            and np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[3]), _bits(b[3])))


def model_frames(case, **kw):
    return [V.model_voxelize(f, c, case["geom"], case["max_points"], case["max_voxels"], **kw)
            for f, c in zip(case["frames"], case["cells"])]


def assert_case_is_sound(oracle, case):
    """The points land in the cells the case was written with, and the oracle equals the numpy restatement."""
    assert V.grid_of(case["geom"]).tolist() == list(case["geom"]["grid"])
    for f, c in zip(case["frames"], case["cells"]):
        assert f.dtype == np.float32 and f.shape == (len(c), case["nfeat"])
        assert np.array_equal(V.cells_of(f, case["geom"]), c)
    want = oracle_frames(oracle, case)
    for a, b in zip(model_frames(case), want):
        assert same(a, b)
    return want


# ----------------------------------------------------------------------------------------------- (a)
def test_cap_in_batch_has_teeth(oracle):
    case = V.cap_in_batch()
    want = assert_case_is_sound(oracle, case)
    distinct = [len(V.first_appearance(c)[0]) for c in case["cells"]]
    assert distinct == [200, 50, 0, 51, 49]
    assert [len(w[1]) for w in want] == [50, 50, 0, 50, 49]
    for b in (0, 3):                                           # the capped frames
        cells = case["cells"][b]
        order, first = V.first_appearance(cells)
        kept, dropped = set(order[:V.CAP].tolist()), set(order[V.CAP:].tolist())
        assert np.array_equal(want[b][1][-1], V.cell_coords_zyx([order[49]], case["geom"])[0])     # number 49 is kept
        later = np.flatnonzero(np.isin(cells, list(dropped)) & (np.arange(len(cells)) > first[V.CAP]))
        assert len(later) >= 2                                  # dropped cells come back ...
        nb = [cells[i - 1] in kept and cells[i + 1] in kept for i in later if 0 < i < len(cells) - 1]
        assert sum(nb) >= 2                                     # ... lane by lane between kept cells
        for variant in ("clamp", "break", "by_cell_id"):
            got = V.model_voxelize(case["frames"][b], cells, case["geom"], case["max_points"], V.CAP, variant=variant)
            assert not same(got, want[b]), (b, variant)
    cells = case["cells"][0]
    c50 = V.first_appearance(cells)[0][50]
    runs = np.diff(np.flatnonzero(np.concatenate([[True], cells[1:] != cells[:-1], [True]])))
    starts = np.cumsum(np.concatenate([[0], runs[:-1]]))
    assert max(r for r, s in zip(runs, starts) if cells[s] == c50) > 128      # a dropped cell's run covers whole waves
    for b in (1, 4):                                           # at and under the cap nothing is cut
        assert same(V.model_voxelize(case["frames"][b], case["cells"][b], case["geom"], 5, 10 ** 6), want[b])


# ----------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("max_points", V.GATHER_MAX_POINTS)
def test_gather_sweep_has_teeth(oracle, max_points):
    for nfeat in V.GATHER_NFEAT:
        case = V.gather_sweep(max_points, nfeat)
        want = assert_case_is_sound(oracle, case)
        for b, w in enumerate(want):
            cells = case["cells"][b]
            counts = np.array([int((cells == c).sum()) for c in V.first_appearance(cells)[0]])
            for size in case["sizes"]:
                assert size == 0 or size in counts
            assert w[2].max() == max_points and counts.max() == 5 * max_points
            big = V.first_appearance(cells)[0][int(np.argmax(counts))]
            assert len(set((np.flatnonzero(cells == big) // 64).tolist())) >= 2   # its points lie in several waves
            got = V.model_voxelize(case["frames"][b], cells, case["geom"], max_points, case["max_voxels"],
                                   arrival=lambda idx: idx[::-1])
            assert not same(got, w), "arrival order kept instead of index order"


def test_voxelizer_refuses_caps_it_cannot_hold():
    """max_points beyond the gather kernels' 32 slots, max_points = 0 and max_voxels = 0 are refused before any launch
    (the pointers are dummies: nothing may be dereferenced on the way to the refusal)."""
    from al3d import lib
    p = ctypes.c_void_p(256)
    g = V.SMALL
    rm, vs = (ctypes.c_float * 3)(*g["range"][:3]), (ctypes.c_float * 3)(*g["vsize"])
    grid = (ctypes.c_int * 3)(*g["grid"])
    for mp, mv, what in ((33, 50, "max_points"), (0, 50, "max_points"), (10, 0, "max_voxels")):
        with pytest.raises(lib.Al3dError, match=what):
            lib.call("al3d_voxelize_mean_f32", p, p, 10, 1, 5, rm, vs, grid, mp, mv, p, p, p, p, p, p, p, p, None)


# ----------------------------------------------------------------------------------------------- (c)
def test_frame_edges_has_teeth(oracle):
    case = V.frame_edges()
    want = assert_case_is_sound(oracle, case)
    assert [len(f) for f in case["frames"]] == V.LENGTHS
    cells, shared = case["cells"], case["shared"]
    assert all(shared in c for c, n in zip(cells, V.LENGTHS) if n)
    flat = np.concatenate(cells)
    frame = np.concatenate([np.full(len(c), b) for b, c in enumerate(cells)])
    at = np.flatnonzero(flat == shared)
    in_wave, across = set(), set()
    for i in at:
        for j in at:
            if 0 < j - i <= 4 and frame[i] != frame[j]:
                (in_wave if i // 64 == j // 64 else across).add(int(j - i))
    assert in_wave == {1, 2, 3, 4} and across
    assert V.lane_skip_leaders(cells, compare_frame=True) == V.true_leaders(cells)
    wrong = V.lane_skip_leaders(cells, compare_frame=False)
    assert wrong != V.true_leaders(cells)
    # frames 1, 6 and 8 start inside a wave, right behind the shared cell in the frame before
    assert sorted(k[0] for k, v in V.true_leaders(cells).items() if k[1] == shared and wrong.get(k) != v) == [1, 6, 8]
    # the concatenation as ONE frame is another result: the shared cell is one voxel there
    g = case["geom"]
    one = oracle.voxelize(np.concatenate(case["frames"]), g["range"][:3], g["vsize"], g["grid"], 5,
                          sum(V.LENGTHS))
    assert len(one[1]) < sum(len(w[1]) for w in want)
    assert int((np.all(one[1] == V.cell_coords_zyx([shared], g)[0], axis=1)).sum()) == 1


def test_empty_frame_cases_are_sound(oracle):
    ends, none = V.empty_frame_cases()
    want = assert_case_is_sound(oracle, ends)
    assert [len(f) for f in ends["frames"]] == [0, 0, 5, 0] and [len(w[1]) for w in want] == [0, 0, 3, 0]
    want = assert_case_is_sound(oracle, none)
    assert [len(f) for f in none["frames"]] == [0, 0, 0] and [len(w[1]) for w in want] == [0, 0, 0]


# ----------------------------------------------------------------------------------------------- (d)
def test_stale_grid_pairs_have_teeth(oracle):
    pairs = dict(V.stale_grid_pairs())
    assert sorted(pairs) == ["batch_sizes", "capped", "tail"]
    for name, calls in pairs.items():
        for case in calls:
            assert_case_is_sound(oracle, case)
            assert len(case["frames"]) <= 8
        for prev, nxt in zip(calls[:-1], calls[1:]):
            shared_frames = 0
            for b in range(min(len(prev["cells"]), len(nxt["cells"]))):
                x, y = prev["cells"][b], nxt["cells"][b]
                xl, yl = V.true_leaders([x]), V.true_leaders([y])
                common = set(xl) & set(yl)
                assert len(common) >= 30 and all(yl[k] > xl[k] for k in common)    # every leader moved up
                clean = V.first_appearance(y)[0].tolist()
                assert V.stale_grid_order(x, y) != clean
                shared_frames += 1
            assert shared_frames >= 1
    x, y = pairs["capped"]
    for b in range(2):
        dropped = V.dropped_by_cap(x["cells"][b], V.CAP)
        assert len(dropped) >= 15
        # a restore pass that only visited the KEPT voxels would leave exactly these behind
        assert V.stale_grid_order(x["cells"][b], y["cells"][b], stale_only=dropped) != \
            V.first_appearance(y["cells"][b])[0].tolist()
    x, y = pairs["tail"]
    assert x["tail"] is not None and len(x["tail"]) >= 50
    tail_cells = V.cells_of(x["tail"], x["geom"])
    assert (tail_cells >= 0).all() and set(tail_cells.tolist()) <= set(y["cells"][1].tolist())
    # had the tail rows been taken for points of the last frame, they would sit in its grid below Y's leaders
    polluted = np.concatenate([x["cells"][1], tail_cells])
    assert V.stale_grid_order(polluted, y["cells"][1], stale_only=set(tail_cells.tolist())) != \
        V.first_appearance(y["cells"][1])[0].tolist()
    sizes = [len(c["frames"]) for c in pairs["batch_sizes"]]
    assert sizes == [3, 8, 1]


# ----------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("name", sorted(V.GEOMETRIES))
def test_cell_arithmetic_has_teeth(oracle, name):
    case = V.cell_arithmetic(name)
    geom = case["geom"]
    pts, cells = case["frames"][0], case["cells"][0]
    assert V.grid_of(geom).tolist() == list(geom["grid"])
    want = oracle_frames(oracle, case)[0]
    # the oracle == the numpy float32 statement: np.floor((p - min) / vs), first-appearance order by np.unique
    order, first = V.first_appearance(cells)
    assert len(order) < case["max_voxels"] and np.array_equal(want[1], V.cell_coords_zyx(order, geom))
    assert same(V.model_voxelize(pts, cells, geom, case["max_points"], case["max_voxels"]), want)
    assert (cells >= 0).sum() > 0.9 * len(cells)
    # every special point is dropped, except the zeros and the positive denormal on KITTI's x = 0 edge
    sp = cells[-case["n_special"]:]
    if name == "kitti":
        x_specials = pts[-case["n_special"]:][5:9, 0]
        assert _bits(x_specials).tolist() == _bits(np.array([-0.0, 0.0, 1e-40, -1e-40], np.float32)).tolist()
        assert (sp[5:8] >= 0).all() and sp[8] == -1 and (np.delete(sp, [5, 6, 7]) == -1).all()
        assert len(set(sp[5:8].tolist())) == 1
        flushed = V.cells_of(pts, geom, "ftz")
        assert flushed[-case["n_special"] + 8] == sp[5]        # -1e-40 flushed to -0: cell 0 instead of -1
        assert not np.array_equal(flushed, cells)
    else:
        assert (sp == -1).all()
    # the wrong arithmetics part from numpy float32 on at least 100 edge values of the x and of the y axis
    for d in (0, 1):
        v = case["sets"][d]
        ref = V.axis_index(v, geom["range"][d], geom["vsize"][d])
        for mode in ("recip", "f64"):
            n = int((V.axis_index(v, geom["range"][d], geom["vsize"][d], mode) != ref).sum())
            print(f"{name} axis {d} {mode}: {n} of {len(v)} edge values differ")
            assert n >= 100, (name, d, mode, n)
    for mode in ("recip", "f64"):
        assert not np.array_equal(V.cells_of(pts, geom, mode), cells)
