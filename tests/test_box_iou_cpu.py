"""CPU suite of the box IoU / NMS ops: the plants of tests/box_iou_cases.py are what they claim to be in float64, the
recorded float32 bands hold, the redrawn shares stay under 1 %, the reference golden agrees with the float64 yardstick
within its own recorded gap, and the host-side argument checks of the entries and of ``selector_ops`` work."""
import ctypes
import os

import numpy as np
import pytest

import box_iou_cases as C

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_iou_eval.npz")


def _iou(a, b, convention="det3d", metric="iou", height="_bev"):
    a, b = np.asarray(a, np.float64)[None], np.asarray(b, np.float64)[None]
    return C.metric_matrix(C.inter_matrix64(a, b, convention), a, b, metric, height)[0, 0]


@pytest.mark.parametrize("convention", C.CONVENTIONS)
def test_plants_are_what_they_claim_in_float64(convention):
    for shift in C.PLACEMENTS:
        seen = set()
        for family, a, b in C.plants(shift):
            seen.add(family)
            v = _iou(a, b, convention)
            if family == "identical":
                assert abs(v - 1.0) < 1e-12
            elif family in ("edge_touch", "corner_touch", "zero_size", "far"):
                assert v == 0.0, (family, v)
            elif family == "inside":
                assert abs(_iou(a, b, convention, "over_b") - 1.0) < 1e-12 and 0 < v < 1
                assert abs(_iou(a, b, convention, "overlap") - float(b[3]) * float(b[4])) < 1e-9
            elif family == "right_angles":
                assert abs(abs(float(a[6]) - float(b[6])) - 1e-4) < 2e-7 and 0.3 < v < 1
            elif family == "sliver":
                assert min(a[3], a[4]) == np.float32(0.01) and 0 < v < 1
        assert seen == {"identical", "edge_touch", "corner_touch", "inside", "right_angles", "sliver", "zero_size", "far"}


def test_the_two_conventions_are_one_rectangle_family():
    """DET3D(w, l, r) is HEADING(l, w, -r - pi/2) (to_pcdet, iou3d_nms_utils.py:29-33): corners as sets, and IoUs."""
    rng = np.random.default_rng(3)
    a, b = C.random_boxes(rng, 20).astype(np.float64), C.random_boxes(rng, 20).astype(np.float64)
    swap = lambda r: np.stack([r[:, 0], r[:, 1], r[:, 2], r[:, 4], r[:, 3], r[:, 5], -r[:, 6] - np.pi / 2], 1)      # noqa: E731
    for row, other in zip(a, swap(a)):
        ca, cb = C.corners64(row, "det3d"), C.corners64(other, "heading")
        assert all(np.abs(cb - p).sum(1).min() < 1e-9 for p in ca)
    x = C.metric_matrix(C.inter_matrix64(a, b, "det3d"), a, b, "iou", "3d")
    y = C.metric_matrix(C.inter_matrix64(swap(a), swap(b), "heading"), swap(a), swap(b), "iou", "3d")
    assert np.abs(x - y).max() < 1e-9 and (x > 0).sum() > 5


def test_pool_covers_both_tile_edges():
    p = C.matrix_pool()
    assert len(p["a"]) >= max(C.SIZES_N) and len(p["b"]) >= max(C.SIZES_M)
    assert set(p["family"][:max(C.SIZES_N)]) >= {"identical", "edge_touch", "inside", "right_angles", "sliver", "zero_size", "far"}


def test_recorded_bands_hold(oracle):
    iou_err, metric_err = C.measure(oracle)
    for got, rec in ((iou_err, C.MEASURED), (metric_err, C.MEASURED_METRIC)):
        assert set(got) == set(rec)
        for k, v in got.items():
            assert 0.8 * rec[k] <= v <= rec[k], (k, v, rec[k])
    assert C.BAND == 4 * max(C.MEASURED.values()) and C.BAND_DECIDE >= C.BAND


def test_decision_bands_and_redrawn_shares():
    c = C.best_case()
    assert c["redrawn_share"] < 0.01
    for same in (False, True):
        for metric, height in (("iou", "_bev"), ("iou", "3d")):
            val, ref = C.best_yardstick(c, metric, height, same)
            assert ref[0, 2, 0] == c["ref_off"][1] - 1 or same          # the last reference tile
            if not same:
                assert ref[0, 2, 1] == 10                                # the lower of the duplicates 10 and 70
            assert (ref[1] == -1).all() and (val[1] == 0).all()          # a frame without reference rows
            assert (ref[0, 0] == -1).all() and (ref[1, 1] == -1).all()  # counts 0 and -2
    assert (c["ref_boxes"][10] == c["ref_boxes"][70]).all()
    for name in C.NMS_CASES:
        n = C.nms_case(name)
        assert n["redrawn_share"] < 0.01, name
        assert all(abs(v - n["thresh"]) > C.BAND_DECIDE for v in n["pair_iou"].values()), name
    assert C.nms_case("chain")["expect"].tolist() == [0, 2, 3]
    assert C.nms_case("duplicates")["expect"].tolist() == [1, 0]
    assert C.nms_case("pre_max_ties")["expect"].tolist() == [1, 0, 2]
    assert C.nms_case("post_max")["expect"].tolist() == [0, 1, 2]
    assert C.nms_case("nan_score")["expect"].tolist() == [2, 1, 4]
    big = C.nms_case("n4096")
    assert 1000 < len(big["expect"]) < 4096


def test_golden_agrees_with_the_float64_yardstick():
    z = np.load(GOLD)
    boxes, query = z["boxes"].astype(np.float64), z["query"].astype(np.float64)
    pad = lambda b: np.stack([b[:, 0], b[:, 1], np.zeros(len(b)), b[:, 2], b[:, 3], np.zeros(len(b)), b[:, 4]], 1)      # noqa: E731
    a, q = pad(boxes), pad(query)
    inter = np.array([C.inter_matrix64(a[i:i + 1], q[i:i + 1], "det3d")[0, 0] for i in range(len(a))])
    for k, (crit, metric) in enumerate(((-1, "iou"), (0, "over_b"), (1, "over_a"), (2, "overlap"))):
        f64 = np.array([C.metric_matrix(inter[i:i + 1, None], a[i:i + 1], q[i:i + 1], metric, "_bev")[0, 0] for i in range(len(a))])
        assert np.abs(f64 - z[f"f64_{crit + 1}"]).max() < 1e-12
        assert np.abs(z[f"ref_{crit + 1}"] - f64).max() <= z["gap"][k]
        # the reference works in float32 on absolute coordinates out to 70 m: a product of two coordinates is ~5000 with an
        # ulp of 5e-4 m^2, against footprints of 0.2 .. 40 m^2.  The other footprint convention, or the criteria 0 / 1 the
        # other way round, would miss by 0.05 and more
        assert z["gap"][k] < 1e-3
    cam = lambda b: np.stack([b[:, 0], b[:, 2], b[:, 1], b[:, 3], b[:, 5], b[:, 4], b[:, 6]], 1).astype(np.float64)      # noqa: E731
    ca, cq = cam(z["cam_boxes"]), cam(z["cam_query"])
    for k, metric in enumerate(("iou", "over_a", "over_b")):
        f64 = np.array([C.metric_matrix(inter[i:i + 1, None], ca[i:i + 1], cq[i:i + 1], metric, "3d_kitti")[0, 0] for i in range(len(a))])
        assert np.abs(f64 - z[f"d3_f64_{k}"]).max() < 1e-12
        assert np.abs(z[f"d3_ref_{k}"] - f64).max() <= z["gap_d3"][k] < 1e-3
    assert len(a) >= 200 and (inter > 0).mean() > 0.9


def test_entries_check_their_arguments_without_gpu():
    from al3d import lib
    so = lib.load()
    p = ctypes.c_void_p(256)
    err = lambda: so.al3d_last_error()                                                # noqa: E731
    assert so.al3d_box_iou_matrix_f32(p, 4, 6, 6, p, 4, 7, 6, 0, 0, 1, 0, p, None) == -1 and b"box_dim" in err()
    assert so.al3d_box_iou_matrix_f32(p, 4, 7, 7, p, 4, 7, 6, 0, 0, 1, 0, p, None) == -1 and b"rot_col" in err()
    assert so.al3d_box_iou_matrix_f32(p, 4, 7, 6, p, 4, 7, 6, 0, 2, 1, 0, p, None) == -1 and b"convention" in err()
    assert so.al3d_box_iou_matrix_f32(p, 4, 7, 6, p, 4, 7, 6, 0, 0, 4, 0, p, None) == -1 and b"metric" in err()
    assert so.al3d_box_iou_matrix_f32(p, 4, 5, 4, p, 4, 5, 4, 1, 0, 1, 1, p, None) == -1 and b"no height" in err()
    assert so.al3d_box_iou_matrix_f32(None, 4, 7, 6, p, 4, 7, 6, 0, 0, 1, 0, p, None) == -1 and b"null pointer" in err()
    assert so.al3d_box_iou_matrix_f32(None, 0, 7, 6, None, 4, 7, 6, 0, 0, 1, 0, None, None) == 0
    assert so.al3d_box_iou_matrix_launch_f32(p, 4, 7, 6, p, 4, 7, 6, 0, 0, 1, 0, p, 129, 256, 1, None) == -1 and b"tile_rows" in err()
    assert so.al3d_box_iou_best_f32(p, p, p, 1, 1, 4, 9, 8, p, p, p, 2, 7, 6, 0, 1, 1, 0, p, p, None, None) == -1 and \
        b"null pointer" in err()
    assert so.al3d_box_iou_best_f32(p, p, p, 1, 1, 0, 9, 8, p, p, p, 2, 7, 6, 0, 1, 1, 0, p, p, p, None) == -1 and b"sizes" in err()
    f = ctypes.c_float(0.3)
    assert so.al3d_nms_boxes_f32(p, p, 4097, 7, 6, 0, 1, 0, f, 0, 0, p, 4097, p, p, None) == -1 and \
        b"at most 4096" in err() and b"4097 candidates" in err()
    assert so.al3d_nms_boxes_f32(p, p, 10, 7, 6, 0, 1, 2, f, 0, 0, p, 10, p, p, None) == -1 and b"mode" in err()
    assert so.al3d_nms_boxes_f32(p, p, 10, 7, 6, 0, 1, 0, f, 0, 0, p, 9, p, p, None) == -1 and b"keep holds" in err()
    assert so.al3d_nms_boxes_f32(p, p, 10, 7, 6, 0, 1, 0, ctypes.c_float(float("nan")), 0, 0, p, 10, p, p, None) == -1
    assert so.al3d_nms_boxes_workspace_bytes(-1) == -1 and so.al3d_nms_boxes_workspace_bytes(10) >= 4096 * 64 * 8


def test_python_surface_refuses_host_tensors_and_bad_names():
    import torch
    from al3d import lib, selector_ops as ops
    import al3d.ops as mirrors
    a = torch.zeros((3, 7))
    with pytest.raises(lib.Al3dError, match="device tensor"):
        ops.box_iou_matrix(a, a)
    with pytest.raises(lib.Al3dError, match="device tensor"):
        ops.nms_boxes(a, torch.zeros(3), 0.3)
    with pytest.raises(lib.Al3dError, match="device tensor"):
        mirrors.iou3d_nms.boxes_iou3d_gpu(a, a)
    with pytest.raises(lib.Al3dError, match="metric"):
        ops.box_iou_matrix(a, a, metric="giou")
    with pytest.raises(lib.Al3dError, match="convention"):
        ops.nms_boxes(a, torch.zeros(3), 0.3, convention="kitti")
    assert set(ops.IOU_METRIC) == {m + h for m in C.METRICS for h in C.HEIGHTS}
    assert (ops.BOX_IOU_TILE_ROWS, ops.BOX_IOU_TILE_COLS) == (C.T_ROWS, C.T_COLS)
    assert callable(mirrors.iou3d.nms_gpu) and callable(mirrors.rotate_iou.d3_box_overlap)
