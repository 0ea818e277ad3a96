"""CPU suite: dynamic voxelization -- the numpy yardstick against the golden fixture of the reference's own layers
(tools/gen_golden_dynamic_voxel.py), the argument checks of the two C entry points (made before any launch), the workspace
bound (no array of 4 bytes per cell), and the function that picks the voxelizer for a ``voxel_generator`` dict."""
import ctypes
import os

import numpy as np
import pytest

import voxel_dynamic_numpy as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "dynamic_voxel.npz"))
    off = z["offsets"]
    frames = [z["points"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return z, frames


def test_fixture_is_the_issue_grid_and_labels_its_standin(fx):
    z, frames = fx
    assert z["grid"].tolist() == [12, 10, 4] and Y.grid_of(z["pc_range"], z["voxel_size"]).tolist() == [12, 10, 4]
    assert "voxel_layer" in str(z["standin"])
    assert int(z["zyx_mean_counts"].max()) > 64          # a voxel beyond the one-lane threshold of the kernel


@pytest.mark.parametrize("order", ["zyx", "xyz"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_yardstick_reproduces_the_fixture(fx, order, reduce):
    z, frames = fx
    r = Y.voxelize_batch(frames, z["pc_range"], z["voxel_size"], order, reduce)
    assert np.array_equal(r["coords"], z[f"{order}_{reduce}_coords"])
    assert np.array_equal(r["feat"].view(np.int32), z[f"{order}_{reduce}_feat"].view(np.int32))
    if order == "zyx":
        assert np.array_equal(r["counts"], z[f"zyx_{reduce}_counts"])


def test_yardstick_point_coords_and_sequential_sum(fx):
    z, frames = fx
    pc = np.concatenate([Y.point_coords(f, z["pc_range"], z["voxel_size"]) for f in frames])
    assert np.array_equal(pc, z["point_coords"])
    # np.add.at is the sequential float32 sum: a plain Python loop gives the same bits
    r = Y.voxelize_frame(frames[0], z["pc_range"], z["voxel_size"], "zyx", "sum")
    acc = np.zeros_like(r["feat"])
    for i, row in enumerate(r["point2voxel"]):
        if row >= 0:
            acc[row] = acc[row] + frames[0][i]
    assert np.array_equal(acc.view(np.int32), r["feat"].view(np.int32))
    # NaN coordinates are dropped; -0.0 < +0.0 for max
    p = np.array([[np.nan, 0, 0, 1, 1], [0.1, 0.1, 0.1, -0.0, 0.0], [0.1, 0.1, 0.1, 0.0, -0.0]], np.float32)
    r = Y.voxelize_frame(p, z["pc_range"], z["voxel_size"], "zyx", "max")
    assert r["point2voxel"].tolist() == [-1, 0, 0] and not np.signbit(r["feat"][0, 3:]).any()


def _call_dynamic(so, **over):
    one = ctypes.c_void_p(256)               # never dereferenced: every check below fails before any launch
    f3, i3 = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int * 3)(4, 4, 4)
    a = dict(points=one, off=one, npts=8, B=1, nfeat=5, rmin=f3, vs=f3, grid=i3, order=0, reduce=1, cap=8, ws=one,
             feat=one, coords=one, counts=one, pc=None, p2v=None, nv=one, rb=one, status=one)
    a.update(over)
    return so.al3d_voxelize_dynamic_f32(a["points"], a["off"], a["npts"], a["B"], a["nfeat"], a["rmin"], a["vs"], a["grid"],
                                        a["order"], a["reduce"], a["cap"], a["ws"], a["feat"], a["coords"], a["counts"],
                                        a["pc"], a["p2v"], a["nv"], a["rb"], a["status"], None)


def test_argument_errors_before_any_launch():
    from al3d import lib
    so = lib.load()
    for key in ("points", "off", "ws", "feat", "coords", "counts", "nv", "rb", "status"):
        assert _call_dynamic(so, **{key: None}) == -1, key
        assert b"null pointer" in so.al3d_last_error()
    for bad in (-1, 2):
        assert _call_dynamic(so, order=bad) == -1 and b"order" in so.al3d_last_error()
    for bad in (-1, 3):
        assert _call_dynamic(so, reduce=bad) == -1 and b"reduce" in so.al3d_last_error()
    assert _call_dynamic(so, nfeat=2) == -1 and b"nfeat" in so.al3d_last_error()
    assert _call_dynamic(so, grid=(ctypes.c_int * 3)(2048, 2048, 512)) == -1 and b"2^31" in so.al3d_last_error()
    assert _call_dynamic(so, grid=(ctypes.c_int * 3)(1 << 11, 1 << 10, 1 << 10)) == -1      # exactly 2^31
    # the second front end
    one = ctypes.c_void_p(256)
    d3 = (ctypes.c_int * 3)(4, 4, 4)
    assert so.al3d_dynamic_scatter_f32(None, one, 4, 5, d3, 0, 4, one, one, one, one, None, one, one, None) == -1
    assert b"null pointer" in so.al3d_last_error()
    assert so.al3d_dynamic_scatter_f32(one, one, 4, 5, d3, 7, 4, one, one, one, one, None, one, one, None) == -1
    assert b"reduce" in so.al3d_last_error()
    big = (ctypes.c_int * 3)(1 << 11, 1 << 10, 1 << 10)
    assert so.al3d_dynamic_scatter_f32(one, one, 4, 5, big, 0, 4, one, one, one, one, None, one, one, None) == -1
    assert b"2^31" in so.al3d_last_error()


def test_workspace_has_no_array_of_four_bytes_per_cell():
    """1.2 M points, batch 4, the 0.075 m grid: an int32 grid would be 4 * 1440 * 1440 * 41 * 4 B = 1.36 GB; the presence
    bits are 42 MB, their group counts 11 MB, the rest is per point."""
    from al3d import lib
    so = lib.load()
    n = so.al3d_voxelize_dynamic_workspace_bytes(1_200_000, 4, 1440, 1440, 41)
    assert 0 < n < 256 * 1024 * 1024, n
    bits = 4 * 1440 * 1440 * 41 // 8
    assert n >= bits
    per_point = (n - bits * 1.26) / 1_200_000
    assert per_point < 150, per_point
    # proportional to the points, not to the cells: twice the points adds less than twice the per-point part
    n2 = so.al3d_voxelize_dynamic_workspace_bytes(2_400_000, 4, 1440, 1440, 41)
    assert n2 - n < 150 * 1_200_000


def test_selection_function_and_example_config():
    from al3d import detector_ops as D
    from al3d.utils import Config
    base = dict(range=[-4, -4, -2, 4, 4, 2], voxel_size=[0.5, 0.5, 1.0])
    assert D.voxelizer_class(dict(base, max_points_in_voxel=10, max_voxel_num=60000)) is D.Voxelizer
    assert D.voxelizer_class(dict(base, max_points_in_voxel=-1, max_voxel_num=-1)) is D.DynamicVoxelizer
    assert D.voxelizer_class(dict(base, max_points_in_voxel=-1, max_voxel_num=60000)) is D.DynamicVoxelizer
    assert D.voxelizer_class(dict(base, max_points_in_voxel=10, max_voxel_num=-1)) is D.DynamicVoxelizer
    with pytest.raises(NotImplementedError, match="dynamic pillar"):
        D.build_voxelizer(dict(base, max_points_in_voxel=-1, max_voxel_num=-1), 1, "cpu", with_points=True)
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_lidar_dynamic_spatial_temporal_feature.py"))
    vg = cfg.voxel_generator
    assert vg.max_points_in_voxel == -1 and vg.max_voxel_num == -1
    assert D.voxelizer_class(vg) is D.DynamicVoxelizer
    hard = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_lidar_spatial_temporal_feature.py"))
    assert D.voxelizer_class(hard.voxel_generator) is D.Voxelizer
    assert list(vg.range) == list(hard.voxel_generator.range) and list(vg.voxel_size) == list(hard.voxel_generator.voxel_size)
    assert cfg.model.bbox_head is None
    # the public mirror is exported
    from al3d.models import DynamicScatter, Voxelization, dynamic_scatter  # noqa: F401
    v = Voxelization([0.5, 0.4, 0.75], [-3.0, -2.0, -1.5, 3.0, 2.0, 1.5], -1)
    assert v.grid_size.tolist() == [12, 10, 4]
