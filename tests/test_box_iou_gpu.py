"""GPU suite of the box IoU / NMS ops (csrc/box_iou.hip) against the float64 yardsticks of tests/box_iou_cases.py.  Values
to 4 x the measured float32 error of their metric (``BAND_METRIC``); keep lists and best rows exactly -- the cases keep every
deciding IoU clear of the band."""
import os

import numpy as np
import pytest
import torch

import box_iou_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_iou_eval.npz")


def _t(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _kind(kind):
    return dict(convention="det3d", layout="xyxyr") if kind == "xyxyr" else dict(convention=kind)


@pytest.mark.parametrize("kind", ("det3d", "heading", "xyxyr"))
def test_matrix_every_metric_at_every_tile_edge(kind):
    from al3d import selector_ops as ops
    y = C.matrix_yardstick(kind)
    heights = ("_bev",) if kind == "xyxyr" else C.HEIGHTS
    a, b = _t(y["a32"]), _t(y["b32"])
    for m in C.METRICS:
        for h in heights:
            ref = C.metric_matrix(y["inter"], y["a"], y["b"], m, h)
            full = ops.box_iou_matrix(a, b, metric=m + h, **_kind(kind))
            err = np.abs(full.cpu().numpy() - ref).max()
            print(f"{kind} {m + h}: max |kernel - f64| {err:.2e}, bound {C.BAND_METRIC[m + h]:.2e}")
            assert err <= C.BAND_METRIC[m + h], (kind, m + h, err)
            full_bits = _bits(full)
            for n in C.SIZES_N:                                 # every size of both tile edges: slices of the full matrix, bit for bit
                for mm in C.SIZES_M:
                    got = ops.box_iou_matrix(a[:n], b[:mm], metric=m + h, **_kind(kind))
                    assert got.shape == (n, mm)
                    assert np.array_equal(_bits(got), full_bits[:n, :mm]), (m + h, n, mm)


@pytest.mark.parametrize("convention", C.CONVENTIONS)
def test_matrix_families(convention):
    """The diagonal of the pool holds the plants: identical boxes give 1, touching, zero-size and far ones exactly 0"""
    from al3d import selector_ops as ops
    p = C.matrix_pool()
    n = len(p["family"])
    got = ops.box_iou_matrix(_t(p["a"]), _t(p["b"][:n]), metric="iou_bev", convention=convention).cpu().numpy()
    seen = set()
    for k, f in enumerate(p["family"]):
        v = got[k, k]
        seen.add(f)
        if f == "identical":
            assert abs(v - 1.0) <= C.BAND
        elif f in ("zero_size", "far"):
            assert v == 0.0
        elif f in ("edge_touch", "corner_touch"):
            assert v <= C.BAND
        else:
            assert 0.0 < v < 1.0
    assert len(seen) == 8


def test_det3d_rows_are_heading_rows_swapped():
    """DET3D(w, l, r) = HEADING(l, w, -r - pi/2) to the band (to_pcdet), and boxes_iou3d_gpu is the float64 3-D IoU"""
    from al3d import selector_ops as ops
    from al3d.ops import iou3d_nms
    y = C.matrix_yardstick("det3d")
    swap = lambda r: np.stack([r[:, 0], r[:, 1], r[:, 2], r[:, 4], r[:, 3], r[:, 5], -r[:, 6] - np.float32(np.pi / 2)], 1)      # noqa: E731
    d = ops.box_iou_matrix(_t(y["a32"]), _t(y["b32"]), metric="iou3d", convention="det3d").cpu().numpy()
    h = ops.box_iou_matrix(_t(swap(y["a32"])), _t(swap(y["b32"])), metric="iou3d", convention="heading").cpu().numpy()
    # the swapped angle is rounded to float32 once more: half an ulp of an angle up to 3 pi / 2 moves a corner of a 12 m box
    # by 1.5e-6 m, far inside the band of the IoU
    assert np.abs(d - h).max() <= 2 * C.BAND_METRIC["iou3d"]
    ref = C.metric_matrix(y["inter"], y["a"], y["b"], "iou", "3d")
    got = iou3d_nms.boxes_iou3d_gpu(_t(y["a32"]), _t(y["b32"]))
    assert got.dtype == torch.float32 and got.is_cuda
    assert np.abs(got.cpu().numpy() - ref).max() <= C.BAND_METRIC["iou3d"]
    bev = iou3d_nms.boxes_iou_bev(_t(y["a32"]), _t(y["b32"])).cpu().numpy()
    yh = C.matrix_yardstick("heading")
    assert np.abs(bev - C.metric_matrix(yh["inter"], yh["a"], yh["b"], "iou", "_bev")).max() <= C.BAND


def test_matrix_nonfinite_rows_give_zero_and_leave_the_rest_alone():
    from al3d import selector_ops as ops
    y = C.matrix_yardstick("det3d")
    rng = np.random.default_rng(5)
    ia, ib = [0, 3, 16, 17, 40], [1, 2, 63, 64, 65, 100, 128]
    a2, b2 = C.nonfinite_rows(y["a32"], ia, rng), C.nonfinite_rows(y["b32"], ib, rng)
    for metric in ("iou_bev", "over_a3d", "overlap3d_kitti"):
        clean = ops.box_iou_matrix(_t(y["a32"]), _t(y["b32"]), metric=metric)
        got = ops.box_iou_matrix(_t(a2), _t(b2), metric=metric)
        assert bool(torch.isfinite(got).all())
        assert bool((got[ia] == 0).all()) and bool((got[:, ib] == 0).all())
        keep_a = np.setdiff1d(np.arange(len(a2)), ia)
        keep_b = np.setdiff1d(np.arange(len(b2)), ib)
        assert np.array_equal(_bits(got)[np.ix_(keep_a, keep_b)], _bits(clean)[np.ix_(keep_a, keep_b)])


def test_matrix_launch_shapes_and_early_reject_keep_the_bits():
    from al3d import selector_ops as ops
    for kind in ("det3d", "xyxyr"):
        y = C.matrix_yardstick(kind)
        a, b = _t(y["a32"]), _t(y["b32"])
        for metric in ("iou_bev", "iou3d") if kind == "det3d" else ("overlap_bev",):
            ref = ops.box_iou_matrix(a, b, metric=metric, **_kind(kind))
            for launch in C.LAUNCH_MATRIX:
                got = ops.box_iou_matrix(a, b, metric=metric, launch=launch, **_kind(kind))
                assert np.array_equal(_bits(got), _bits(ref)), (kind, metric, launch)
    again = ops.box_iou_matrix(a, b, metric="overlap_bev", **_kind("xyxyr"))
    assert np.array_equal(_bits(again), _bits(ref))


# ---------------------------------------------------------------- best IoU per detection
def _best_args(c):
    return (_t(c["boxes"]), _t(c["labels"], torch.int32), _t(c["counts"], torch.int32), _t(c["ref_boxes"]),
            _t(c["ref_labels"], torch.int32), _t(c["ref_off"], torch.int32))


@pytest.mark.parametrize("same_class", (False, True))
@pytest.mark.parametrize("metric", ("iou_bev", "iou3d"))
def test_best_iou_equals_the_yardstick_and_the_matrix_maximum(metric, same_class):
    from al3d import selector_ops as ops
    c = C.best_case()
    args = _best_args(c)
    val, ref = ops.box_iou_best(*args, metric=metric, same_class=same_class)
    want_val, want_ref = C.best_yardstick(c, "iou", "_bev" if metric == "iou_bev" else "3d", same_class)
    assert np.array_equal(ref.cpu().numpy(), want_ref)
    err = np.abs(val.cpu().numpy() - want_val).max()
    print(f"best {metric} same_class={same_class}: max |kernel - f64| {err:.2e}, bound {C.BAND_METRIC[metric]:.2e}")
    assert err <= C.BAND_METRIC[metric]
    # bit for bit the row maximum of the matrix entry on the frame, the lowest row among equal maxima
    B, nt, post = c["B"], c["nt"], c["post"]
    for b in range(B):
        r0, r1 = int(c["ref_off"][b]), int(c["ref_off"][b + 1])
        m = ops.box_iou_matrix(args[0][b].reshape(nt * post, 9), args[3][r0:r1], metric=metric, rot_col=8, rot_col_b=6).cpu().numpy()
        for s in range(nt * post):
            t, i = divmod(s, post)
            if i >= min(max(int(c["counts"][b, t]), 0), post):
                assert ref[b, t, i] == -1 and val[b, t, i] == 0
                continue
            cand = np.arange(r1 - r0)
            if same_class:
                cand = cand[c["ref_labels"][r0:r1] == c["labels"][b, t, i]]
            if not len(cand):
                assert ref[b, t, i] == -1 and val[b, t, i] == 0
                continue
            k = cand[np.argmax(m[s, cand])]
            assert int(ref[b, t, i]) == r0 + k
            assert np.float32(val[b, t, i].item()).view(np.int32) == m[s, k].view(np.int32)


def test_best_iou_launch_shapes_keep_the_bits_and_bad_offsets_raise():
    from al3d import lib, selector_ops as ops
    c = C.best_case()
    args = _best_args(c)
    for same in (False, True):
        val, ref = ops.box_iou_best(*args, metric="iou3d", same_class=same)
        for launch in C.LAUNCH_BEST:
            v2, r2 = ops.box_iou_best(*args, metric="iou3d", same_class=same, launch=launch)
            assert np.array_equal(_bits(v2), _bits(val)) and torch.equal(r2, ref), launch
    for bad in ([0, 5, 3, 194], [0, 193, 193, 195], [-1, 193, 193, 194]):
        with pytest.raises(lib.Al3dError, match="not ascending"):
            ops.box_iou_best(*args[:5], _t(np.asarray(bad), torch.int32))


# ---------------------------------------------------------------- NMS
def _nms(c, **kw):
    from al3d import selector_ops as ops
    return ops.nms_boxes(_t(c["boxes"]), _t(c["scores"]), c["thresh"], pre_max=c["pre_max"], post_max=c["post_max"],
                         mode=c["mode"], convention=c["convention"], **kw)


@pytest.mark.parametrize("name", C.NMS_CASES)
def test_nms_keeps_what_the_float64_loop_keeps(name):
    c = C.nms_case(name)
    keep = _nms(c)
    assert keep.dtype == torch.int64 and keep.is_cuda
    assert keep.cpu().numpy().tolist() == c["expect"].tolist()
    if c["n"] in (65, 4096):
        for launch in C.LAUNCH_NMS:
            assert torch.equal(_nms(c, launch=launch), keep), launch


def test_nms_normal_mode_differs_from_rotated_on_rotated_boxes():
    c = dict(C.nms_case("normal"))
    normal = _nms(c)
    c["mode"] = "rotated"
    rotated = _nms(c)
    assert normal.cpu().numpy().tolist() == C.nms_case("normal")["expect"].tolist()
    assert normal.cpu().numpy().tolist() != rotated.cpu().numpy().tolist()


def test_nms_nonfinite_and_degenerate_boxes_neither_suppress_nor_fall():
    """A box with an inf, a NaN or a zero size has IoU 0 with everything: it is kept (at its rank) and what it covered
    lives; every other decision stays what the float64 loop gives without that box's pairs."""
    c = dict(C.nms_case("n65"))
    boxes = c["boxes"].copy()
    hit = sorted({i for pair, v in c["pair_iou"].items() if v > c["thresh"] for i in pair})[:3]
    assert len(hit) == 3
    boxes[hit[0], 0], boxes[hit[1], 6], boxes[hit[2], 3] = np.inf, np.nan, 0.0
    pairs = {k: v for k, v in c["pair_iou"].items() if not set(k) & set(hit)}
    want = C.nms64(C._SparseIou(pairs), c["scores"], c["thresh"])
    assert set(hit) <= set(want.tolist()) and want.tolist() != c["expect"].tolist()
    c["boxes"] = boxes
    assert _nms(c).cpu().numpy().tolist() == want.tolist()


def test_nms_refuses_4097_candidates():
    from al3d import lib, selector_ops as ops
    c = C.nms_case("n4097_pre4096")
    with pytest.raises(lib.Al3dError, match="4097 candidates.*at most 4096"):
        ops.nms_boxes(_t(c["boxes"]), _t(c["scores"]), c["thresh"])
    so = lib.load()
    b, s = _t(c["boxes"]), _t(c["scores"])
    keep = torch.empty(4097, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(so.al3d_nms_boxes_workspace_bytes(4097)), dtype=torch.uint8, device=DEV)
    rc = so.al3d_nms_boxes_f32(b.data_ptr(), s.data_ptr(), 4097, 7, 6, 0, 1, 0, 0.3, 0, 0, keep.data_ptr(), 4097,
                               keep.data_ptr(), ws.data_ptr(), None)
    assert rc == -1 and b"at most 4096" in so.al3d_last_error()


# ---------------------------------------------------------------- mirrors
def test_mirrors_keep_the_reference_signatures():
    from al3d.ops import iou3d, iou3d_nms, rotate_iou
    c = C.nms_case("n65")
    keep, none = iou3d_nms.nms_gpu(_t(c["boxes"]), _t(c["scores"]), c["thresh"])
    assert none is None and keep.dtype == torch.int64 and keep.is_cuda
    assert keep.cpu().numpy().tolist() == c["expect"].tolist()
    keep2, _ = iou3d_nms.nms_gpu(_t(c["boxes"]), _t(c["scores"]), c["thresh"], pre_maxsize=10)
    assert set(keep2.cpu().numpy().tolist()) <= set(C.score_order(c["scores"])[:10].tolist())
    n = C.nms_case("normal")
    keep3, none = iou3d_nms.nms_normal_gpu(_t(n["boxes"]), _t(n["scores"]), n["thresh"])
    assert none is None and keep3.cpu().numpy().tolist() == n["expect"].tolist()
    # mmdet3d rows: the chain, as [x1, y1, x2, y2, r]
    ch = C.nms_case("chain")
    x, _ = C.xyxyr_rows(ch["boxes"])
    k = iou3d.nms_gpu(_t(x), _t(ch["scores"]), ch["thresh"], pre_maxsize=None, post_max_size=2)
    assert k.dtype == torch.int64 and k.cpu().numpy().tolist() == ch["expect"].tolist()[:2]
    assert iou3d.nms_normal_gpu(_t(x), _t(ch["scores"]), ch["thresh"]).cpu().numpy().tolist() == ch["expect"].tolist()
    y = C.matrix_yardstick("xyxyr")
    got = iou3d.boxes_iou_bev(_t(y["a32"]), _t(y["b32"])).cpu().numpy()
    assert np.abs(got - C.metric_matrix(y["inter"], y["a"], y["b"], "iou", "_bev")).max() <= C.BAND
    # numpy in, numpy out in the input dtype
    z = np.load(GOLD)
    for dt in (np.float32, np.float64):
        out = rotate_iou.rotate_iou_gpu_eval(z["boxes"][:9].astype(dt), z["query"][:5].astype(dt))
        assert isinstance(out, np.ndarray) and out.dtype == dt and out.shape == (9, 5)
    assert rotate_iou.rotate_iou_gpu_eval(z["boxes"][:0], z["query"][:5]).shape == (0, 5)


def test_eval_mirror_against_the_reference_golden():
    """|kernel - reference| <= the golden's own gap to float64 + the band: pins rbbox_to_corners' convention, the query-first
    argument order of criteria 0 / 1 and the KITTI height rule"""
    from al3d.ops import rotate_iou
    z = np.load(GOLD)
    n = len(z["boxes"])
    d = np.arange(n)
    for k, metric in enumerate(("iou_bev", "over_b_bev", "over_a_bev", "overlap_bev")):
        got = rotate_iou.rotate_iou_gpu_eval(z["boxes"], z["query"], criterion=k - 1)[d, d]
        err = np.abs(got - z[f"ref_{k}"]).max()
        print(f"criterion {k - 1}: max |kernel - reference| {err:.2e}, gap {z['gap'][k]:.2e}, band {C.BAND_METRIC[metric]:.2e}")
        assert err <= z["gap"][k] + C.BAND_METRIC[metric]
        assert np.abs(rotate_iou.bev_box_overlap(z["boxes"], z["query"], k - 1)[d, d] - got).max() == 0
    for k, metric in enumerate(("iou3d_kitti", "over_a3d_kitti", "over_b3d_kitti")):
        got = rotate_iou.d3_box_overlap(z["cam_boxes"], z["cam_query"], criterion=k - 1)[d, d]
        err = np.abs(got - z[f"d3_ref_{k}"]).max()
        print(f"d3 criterion {k - 1}: max |kernel - reference| {err:.2e}, gap {z['gap_d3'][k]:.2e}")
        assert err <= z["gap_d3"][k] + C.BAND_METRIC[metric]
