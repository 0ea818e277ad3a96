"""CPU suite of the ground-truth database builder: the host halves against tests/golden/gt_database.npz, which is the
output of the reference's own ``create_groundtruth_database`` and ``points_in_rbbox`` (tools/gen_golden_gt_database.py).

* ``detector_ops.box_planes`` == the reference's ``surface_equ_3d_jitv2`` planes, bit for bit;
* the numpy yardstick of tests/gt_database_numpy.py == the reference's masks, files and dbinfos (it is what the GPU tests
  compare with at sizes the golden does not have);
* the package's file-name / dbinfo assembly and its writers, fed the golden's masks == the golden, byte for byte;
* the refusals: the CLI without a suffix, the datasets and options that are not built, bad launch shapes (checked before
  any launch, so without a GPU)."""
import ctypes
import importlib.util
import os
import pickle

import numpy as np
import pytest

import gt_database_numpy as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    """Bit for bit; where both are NaN any NaN will do (the edge block's NaN box)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan])


@pytest.mark.parametrize("block", ("f0", "f1", "f2", "edge"))
def test_box_planes_equal_the_reference_planes_bit_for_bit(block):
    from al3d.detector_ops import box_planes
    g = Y.golden()
    with np.errstate(invalid="ignore"):
        planes = box_planes(g[f"{block}_boxes"])
    assert planes.dtype == np.float32 and planes.shape == g[f"{block}_planes"].shape
    assert _same_bits(planes, g[f"{block}_planes"])
    if block == "edge":
        zero = planes[2]                                     # the zero-size box: n = 0 and d = +-0, so sign = 0 everywhere
        assert np.all(zero == 0)


def test_box_planes_refuses_other_dtypes_and_shapes():
    from al3d import lib
    from al3d.detector_ops import box_planes
    with pytest.raises(lib.Al3dError):
        box_planes(np.zeros((3, 9), np.float64))
    with pytest.raises(lib.Al3dError):
        box_planes(np.zeros((3, 6), np.float32))
    assert box_planes(np.zeros((0, 9), np.float32)).shape == (0, 6, 4)


@pytest.mark.parametrize("block", ("f0", "f1", "f2", "edge"))
def test_yardstick_masks_equal_the_reference_masks(block):
    g = Y.golden()
    m = Y.mask(g[f"{block}_points"], g[f"{block}_planes"])
    assert m.shape == g[f"{block}_mask"].shape and np.array_equal(m, g[f"{block}_mask"])


def test_golden_has_the_cases_the_issue_names():
    g = Y.golden()
    assert [len(g[f"f{f}_boxes"]) for f in range(3)] == [70, 0, 14]
    assert all(len(g[f"f{f}_points"]) <= 2100 for f in range(3))
    e = g["edge_mask"]
    assert e[0, 0] and e[1, 0] and e[1, 1]                   # inside one box / inside two overlapping boxes
    assert not e[2:11, 0].any()                              # on a face, an edge, a corner: sign == 0 is outside
    assert not e[~np.isnan(g["edge_points"][:, :3]).any(1), 2].any()       # the zero-size box holds no finite point
    assert e[13:16].all() and e[:, 4].all()                  # a NaN point is in every box, a NaN box holds every point
    counts = np.concatenate([g[f"f{f}_mask"].sum(0) for f in range(3)])
    assert (counts == 0).sum() >= 3 and counts.max() >= 20   # empty objects and full ones


@pytest.mark.parametrize("variant", ("db", "alt"))
def test_yardstick_database_equals_the_reference_database(variant):
    g = Y.golden()
    stem = f"gt_database_{int(g['nsweeps'])}sweeps_withvelo_{g['suffix']}"
    kw = {} if variant == "db" else dict(used_classes=g["used_classes"].tolist(), relative_path=False)
    files, db = Y.database(Y.golden_frames(g), stem, "{root}/alt_db", **kw)
    want = Y.golden_files(g)
    assert list(files) and sorted(files) == sorted(want)
    for n, a in want.items():
        assert files[n].dtype == np.float32 and files[n].tobytes() == a.tobytes(), n
    Y.assert_dbinfos(pickle.loads(pickle.dumps(db)), g, variant)


@pytest.mark.parametrize("variant", ("db", "alt"))
def test_package_assembly_fed_the_golden_masks_reproduces_the_golden(variant, tmp_path):
    from al3d.datasets.create_gt_database import GtDatabaseWriter, database_paths
    g = Y.golden()
    if variant == "db":
        db_path, dbinfo_path = database_paths(tmp_path, int(g["nsweeps"]), str(g["suffix"]))
        assert db_path.name == "gt_database_3sweeps_withvelo_g" and dbinfo_path.name == "dbinfos_train_3sweeps_withvelo_g.pkl"
        w = GtDatabaseWriter(db_path, dbinfo_path)
    else:
        db_path, dbinfo_path = tmp_path / "alt_db", tmp_path / "alt.pkl"
        w = GtDatabaseWriter(db_path, dbinfo_path, relative_path=False, used_classes=g["used_classes"].tolist())
    for f, (points, boxes, names, _) in enumerate(Y.golden_frames(g)):
        rows = []
        for i in range(len(boxes)):
            r = points[g[f"f{f}_mask"][:, i]]
            r[:, :3] -= boxes[i, :3]
            rows.append(r)
        w.add_frame(f, names, boxes, rows)
        assert not dbinfo_path.exists()                      # the pickle comes last
    w.close()
    Y.assert_files(db_path, g)
    with open(dbinfo_path, "rb") as fh:
        Y.assert_dbinfos(pickle.load(fh), g, variant, root=tmp_path)
    assert not os.path.exists(str(dbinfo_path) + ".tmp")


def test_database_paths_without_a_suffix():
    from al3d.datasets.create_gt_database import database_paths
    db, pkl = database_paths("/data/nusc", 10)
    assert str(db) == "/data/nusc/gt_database_10sweeps_withvelo" and str(pkl) == "/data/nusc/dbinfos_train_10sweeps_withvelo.pkl"
    db, pkl = database_paths("/data/nusc", 10, "600", dbinfo_path="/x/y.pkl")
    assert str(db) == "/data/nusc/gt_database_10sweeps_withvelo_600" and str(pkl) == "/x/y.pkl"


def test_a_failed_write_leaves_no_pickle(tmp_path, monkeypatch):
    from al3d.datasets import create_gt_database as M
    pkl = tmp_path / "dbinfos.pkl"
    pkl.write_bytes(b"stale")
    w = M.GtDatabaseWriter(tmp_path / "db", pkl)
    assert not pkl.exists()                                  # an earlier run's pickle does not vouch for this run's files

    def boom(path, rows):
        raise OSError("disk full")

    monkeypatch.setattr(M, "_write_bin", boom)
    w.add_frame(0, np.array(["car"]), np.zeros((1, 9), np.float32), [np.zeros((2, 5), np.float32)])
    with pytest.raises(OSError):
        w.close()
    assert not pkl.exists() and not os.path.exists(str(pkl) + ".tmp")


def _create_data():
    spec = importlib.util.spec_from_file_location("al3d_create_data", os.path.join(ROOT, "tools", "create_data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_refuses_without_a_suffix(tmp_path):
    cli = _create_data()
    with pytest.raises(SystemExit) as e:
        cli.main(["nuscenes_data_prep", "--root_path", str(tmp_path), "--version", "v1.0-mini"])
    assert "devkit" in str(e.value) and "--suffix" in str(e.value)
    assert os.listdir(tmp_path) == []
    with pytest.raises(SystemExit):                          # argparse: --version is required, as in the reference's signature
        cli.main(["nuscenes_data_prep", "--root_path", str(tmp_path)])


@pytest.mark.parametrize("args, kwargs, word", [
    (("KITTI", "/nowhere"), {}, "KITTI"), (("LYFT", "/nowhere"), {}, "LYFT"),
    (("NUSC", "/nowhere"), dict(add_rgb=True), "add_rgb"), (("NUSC", "/nowhere"), dict(bev_only=True), "bev_only")])
def test_what_is_not_built_says_so(args, kwargs, word):
    from al3d.datasets import create_groundtruth_database
    with pytest.raises(NotImplementedError) as e:
        create_groundtruth_database(*args, **kwargs)
    assert word in str(e.value) and "not built" in str(e.value)


def test_signature_and_defaults_are_the_reference_ones():
    import inspect
    from al3d.datasets import create_groundtruth_database
    sig = inspect.signature(create_groundtruth_database)
    assert [(n, p.default) for n, p in sig.parameters.items() if p.kind == p.POSITIONAL_OR_KEYWORD] == [
        ("dataset_class_name", inspect.Parameter.empty), ("data_path", inspect.Parameter.empty), ("info_path", None),
        ("used_classes", None), ("db_path", None), ("dbinfo_path", None), ("relative_path", True), ("add_rgb", False),
        ("lidar_only", False), ("bev_only", False), ("coors_range", None)]
    assert any(p.kind == p.VAR_KEYWORD for p in sig.parameters.values())


def test_points_in_rbbox_refuses_other_axes_and_origins():
    import al3d.ops
    p, b = np.zeros((1, 3), np.float32), np.zeros((1, 7), np.float32)
    with pytest.raises(NotImplementedError):
        al3d.ops.points_in_rbbox(p, b, z_axis=1)
    with pytest.raises(NotImplementedError):
        al3d.ops.points_in_rbbox(p, b, origin=(0.5, 0.5, 0))
    with pytest.raises(TypeError):
        al3d.ops.points_in_rbbox(p.astype(np.float64), b)


def test_entries_check_their_arguments_before_any_launch():
    from al3d import lib
    so = lib.load()
    p = ctypes.c_void_p(256)
    assert so.al3d_points_in_boxes_workspace_bytes(10, 32, 256) >= 256 + 10 * 128 * 4
    for bad in ((10, 0, 256), (10, 1025, 256), (10, 32, 96), (-1, 32, 256), (1 << 31, 32, 256)):
        assert so.al3d_points_in_boxes_workspace_bytes(*bad) == -1
    count = (p, 8, 5, p, 1, p, p, 2, p, p, p)
    for shape in ((0, 256, 64), (32, 100, 64), (32, 256, 0), (32, 256, 65)):
        assert so.al3d_points_in_boxes_count_launch_f32(*count, *shape, None) == -1
        assert b"threads 64 / 128 / 256" in so.al3d_last_error()
    assert so.al3d_points_in_boxes_count_f32(p, 8, 2, p, 1, p, p, 2, p, p, p, None) == -1          # F < 3
    assert so.al3d_points_in_boxes_count_f32(p, 8, 5, p, 65536, p, p, 2, p, p, p, None) == -1      # frames
    assert so.al3d_points_in_boxes_count_f32(p, 8, 5, p, 1, p, p, 2, p, p, None, None) == -1       # no status word
    assert b"null pointer" in so.al3d_last_error()
    gather = (p, 8, 5, p, 1, p, p, 2, p, p, p, p)
    assert so.al3d_points_in_boxes_gather_f32(*gather, 6, p, 4, p, None) == -1                     # F_out > F
    assert so.al3d_points_in_boxes_gather_f32(*gather, 2, p, 4, p, None) == -1                     # F_out < 3
    assert so.al3d_points_in_boxes_gather_f32(*gather, 5, p, -1, p, None) == -1                    # T < 0
    assert so.al3d_points_in_boxes_mask_launch_u8(p, 8, 5, p, 2, p, 32, 64, None) == -1
    assert so.al3d_points_in_boxes_mask_u8(p, -1, 5, p, 2, p, None) == -1
    assert so.al3d_points_in_boxes_mask_u8(None, 0, 5, None, 0, None, None) == 0                   # nothing to do, nothing touched
