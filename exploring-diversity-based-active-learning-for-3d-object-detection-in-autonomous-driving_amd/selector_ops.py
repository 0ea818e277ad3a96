"""Device-side selector primitives: torch tensors in, HIP kernels underneath.

PyTorch is plumbing here (device memory + the current stream); every number is
produced by libal3d_hip.so.  All functions require CUDA(ROCm) tensors and raise
if handed CPU ones -- there is no host fallback.
"""
import torch

from . import lib

NORMALIZE = {None: 0, "none": 0, "exp": 1, "linear": 2}
SHARD_MIN_ROWS = 4096          # pools below this are cheaper to map on every rank than to gather
AGGREGATE = {"sum": 0, "min": 1, "max": 2}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, dtype, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise lib.Al3dError(f"{name}: expected a device tensor (no CPU fallback)")
    if t.dtype != dtype:
        raise lib.Al3dError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def l1_distance(feats, p=2, shard=True):
    """[N,C] f32 embeddings -> [N,N] f32 L1 map (feature_selector.py:87-109).

    Under torch.distributed (and ``shard``) this is a COLLECTIVE: every rank computes one block of
    rows and the blocks are all-gathered, so every rank must call it.  ``shard=False`` computes the
    whole map locally (what a rank-0-only checker needs)."""
    import torch.distributed as dist
    feats = _dev(feats, torch.float32, "feats")
    n, c = feats.shape
    if (not shard or not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1
            or n < SHARD_MIN_ROWS):
        out = torch.empty((n, n), dtype=torch.float32, device=feats.device)
        lib.call("al3d_l1_distance_f32", _ptr(feats), n, c, int(p), _ptr(out), _stream())
        return out
    # N>1: every rank holds all embeddings (they were all-gathered); each computes a block of rows
    world, rank = dist.get_world_size(), dist.get_rank()
    per = (n + world - 1) // world
    r0 = min(n, rank * per)
    nrows = min(n, r0 + per) - r0
    block = torch.empty((per, n), dtype=torch.float32, device=feats.device)
    lib.call("al3d_l1_distance_rows_f32", _ptr(feats), n, c, int(p), r0, nrows, _ptr(block), _stream())
    full = torch.empty((world * per, n), dtype=torch.float32, device=feats.device)
    dist.all_gather_into_tensor(full, block)
    return full[:n]


def combine_maps(n, spatial=None, temporal_id=None, feat=None, normalize="exp", aggregate="sum",
                 lambda_t=1.0, lambda_f=1.0, spatial_scale=1.0, temporal_scale=1.0, device=None):
    spatial = _dev(spatial, torch.float64, "spatial")
    temporal_id = _dev(temporal_id, torch.int64, "temporal_id")
    feat = _dev(feat, torch.float32, "feat")
    for t in (spatial, temporal_id, feat):
        if t is not None:
            device = t.device
    out = torch.empty((n, n), dtype=torch.float64, device=device)
    lib.call("al3d_combine_maps_f64", _ptr(spatial), _ptr(temporal_id), _ptr(feat), n,
             NORMALIZE[normalize], AGGREGATE[aggregate], float(lambda_t), float(lambda_f),
             float(spatial_scale), float(temporal_scale), _ptr(out), _stream())
    return out


def euclid_map(xy, loc_id):
    """EuSpatialSelector map (euclidean_spatial_selector.py:95-106)."""
    xy = _dev(xy, torch.float64, "xy")
    loc_id = _dev(loc_id, torch.int64, "loc_id")
    n = xy.shape[0]
    out = torch.empty((n, n), dtype=torch.float64, device=xy.device)
    lib.call("al3d_euclid_map_f64", _ptr(xy), _ptr(loc_id), n, _ptr(out), _stream())
    return out


def max_finite(a):
    a = _dev(a, torch.float64, "a")
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    lib.call("al3d_max_finite_f64", _ptr(a), a.numel(), _ptr(out), _stream())
    return float(out.item())


def knn_2d(xy, kq):
    xy = _dev(xy, torch.float64, "xy")
    n = xy.shape[0]
    d = torch.empty((n, kq), dtype=torch.float64, device=xy.device)
    i = torch.empty((n, kq), dtype=torch.int64, device=xy.device)
    lib.call("al3d_knn_2d_f64", _ptr(xy), n, int(kq), _ptr(d), _ptr(i), _stream())
    return d, i


def apsp_knn(knn_d, knn_i, row0=0, nrows=None):
    """Geodesic rows [row0, row0+nrows) of the kNN graph, f64 [nrows, n]."""
    knn_d = _dev(knn_d, torch.float64, "knn_d")
    knn_i = _dev(knn_i, torch.int64, "knn_i")
    n, kq = knn_d.shape
    nrows = n - row0 if nrows is None else nrows
    out = torch.empty((nrows, n), dtype=torch.float64, device=knn_d.device)
    if nrows == 0 and 0 <= row0 <= n:
        return out      # an empty block has no storage (data_ptr() is null): nothing to hand over
    ws = torch.empty(max(1, lib.load().al3d_apsp_workspace_bytes(n, kq)), dtype=torch.uint8,
                     device=knn_d.device)
    lib.call("al3d_apsp_knn_rows_f64", _ptr(knn_d), _ptr(knn_i), n, kq, int(row0), int(nrows), _ptr(out),
             _ptr(ws), _stream())
    return out


def spatial_map(xy, k=8):
    """kNN(k)-graph geodesic map, f64 [N,N] (spatial_temporal_selector.py:92-104).

    Under torch.distributed the N source rows are sharded over the ranks (each computes a
    contiguous block) and all-gathered -- the sweeps are independent per source.  That makes this a
    COLLECTIVE (every rank must call it); ``knn_2d`` + ``apsp_knn`` is the local form."""
    import torch.distributed as dist
    d, i = knn_2d(xy, k + 1)
    n = d.shape[0]
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1 or n < SHARD_MIN_ROWS:
        return apsp_knn(d, i)
    world, rank = dist.get_world_size(), dist.get_rank()
    per = (n + world - 1) // world
    r0 = min(n, rank * per)
    rows = apsp_knn(d, i, r0, min(n, r0 + per) - r0)
    pad = torch.empty((per, n), dtype=torch.float64, device=d.device)
    pad[: rows.shape[0]] = rows
    full = torch.empty((world * per, n), dtype=torch.float64, device=d.device)
    dist.all_gather_into_tensor(full, pad)
    return full[:n]


def frame_entropy(scores, counts):
    """scores [B,nt,post] f32, counts [B,nt] i32 -> [B] mean binary entropy per frame."""
    scores = _dev(scores, torch.float32, "scores")
    counts = _dev(counts, torch.int32, "counts")
    B, nt, post = scores.shape
    out = torch.empty((B,), dtype=torch.float32, device=scores.device)
    lib.call("al3d_frame_entropy_f32", _ptr(scores), _ptr(counts), B, nt, post, _ptr(out), _stream())
    return out


def frame_weighted_entropy(scores, labels, counts, class_weight):
    scores = _dev(scores, torch.float32, "scores")
    labels = _dev(labels, torch.int32, "labels")
    counts = _dev(counts, torch.int32, "counts")
    cw = _dev(class_weight, torch.float32, "class_weight")
    B, nt, post = scores.shape
    out = torch.empty((B,), dtype=torch.float32, device=scores.device)
    lib.call("al3d_frame_weighted_entropy_f32", _ptr(scores), _ptr(labels), _ptr(counts), B, nt, post,
             _ptr(cw), cw.numel(), _ptr(out), _stream())
    return out


MATCH_TOO_MANY_BOXES, MATCH_CLASS_TOO_LARGE, MATCH_BAD_OFFSETS = 1, 2, 4      # AL3D_MATCH_* of include/al3d.h


def _view4(view):
    """``(flip_x, flip_y, rot, scale)`` -> the four host floats of the C ABI (None stays None: the identity)."""
    if view is None:
        return None
    fx, fy, rot, scale = view
    return (lib.c_flt * 4)(1.0 if fx else 0.0, 1.0 if fy else 0.0, float(rot), float(scale))


def match_boxes(boxes, scores, labels, counts, ref_boxes, ref_labels, ref_scores, ref_off, ncls, dist_th=1.0,
                max_boxes=500, class_range=None, origin=None, view=None):
    """The nuScenes matching rule per frame (classwise_weight/algo.py:36-106) on the raw NMS buffers.

    ``boxes [B,nt,post,D]`` f32, ``scores`` / ``labels [B,nt,post]`` f32 / i32, ``counts [B,nt]`` i32; reference boxes
    concatenated by frame: ``ref_boxes [R,>=6]`` f32, ``ref_labels [R]`` i32, ``ref_scores [R]`` f32, ``ref_off [B+1]`` i32.
    ``class_range [ncls]`` + ``origin [B,2]``: the range rule of the devkit's ``filter_eval_boxes``; ``view`` =
    ``(flip_x, flip_y, rot, scale)``: the predictions come from a cloud augmented by ``points_view_`` and are mapped back.
    Returns ``dict(match_ref [B,nt,post] i32, match_iou [B,nt,post] f32, cls_count [B,ncls] i32, cls_quality, cls_cons
    [B,ncls] f32)``; see ``al3d_match_boxes_f32`` in include/al3d.h.  Reads the status word back (one small D2H) and raises
    ``AssertionError`` for a frame with more than ``max_boxes`` predictions, as the devkit's ``load_prediction`` does.

    Not built: the bike-rack and ``num_pts == 0`` filters of ``filter_eval_boxes`` (they need devkit tables the infos files
    do not carry) and the lidar -> global conversion (centre distance and scale IoU are invariant under it)."""
    boxes = _dev(boxes, torch.float32, "boxes")
    scores = _dev(scores, torch.float32, "scores")
    labels = _dev(labels, torch.int32, "labels")
    counts = _dev(counts, torch.int32, "counts")
    ref_boxes = _dev(ref_boxes, torch.float32, "ref_boxes")
    ref_labels = _dev(ref_labels, torch.int32, "ref_labels")
    ref_scores = _dev(ref_scores, torch.float32, "ref_scores")
    ref_off = _dev(ref_off, torch.int32, "ref_off")
    class_range = _dev(class_range, torch.float32, "class_range")
    origin = _dev(origin, torch.float32, "origin")
    if boxes.dim() != 4 or scores.shape != boxes.shape[:3] or labels.shape != boxes.shape[:3] or \
            counts.shape != boxes.shape[:2]:
        raise lib.Al3dError("match_boxes: boxes [B,nt,post,D], scores / labels [B,nt,post], counts [B,nt] expected")
    B, nt, post, bd = boxes.shape
    R = ref_boxes.shape[0]
    if ref_boxes.dim() != 2 or ref_labels.shape != (R,) or ref_scores.shape != (R,) or ref_off.shape != (B + 1,):
        raise lib.Al3dError("match_boxes: ref_boxes [R,>=6], ref_labels / ref_scores [R], ref_off [B+1] expected")
    if (class_range is None) != (origin is None):
        raise lib.Al3dError("match_boxes: class_range and origin go together")
    if class_range is not None and (class_range.shape != (ncls,) or origin.shape != (B, 2)):
        raise lib.Al3dError("match_boxes: class_range [ncls] and origin [B,2] expected")
    dev = boxes.device
    out = dict(match_ref=torch.empty((B, nt, post), dtype=torch.int32, device=dev),
               match_iou=torch.empty((B, nt, post), dtype=torch.float32, device=dev),
               cls_count=torch.empty((B, ncls), dtype=torch.int32, device=dev),
               cls_quality=torch.empty((B, ncls), dtype=torch.float32, device=dev),
               cls_cons=torch.empty((B, ncls), dtype=torch.float32, device=dev))
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    lib.call("al3d_match_boxes_f32", _ptr(boxes), _ptr(scores), _ptr(labels), _ptr(counts), B, nt, post, bd,
             _ptr(ref_boxes) if R else None, _ptr(ref_labels) if R else None, _ptr(ref_scores) if R else None,
             _ptr(ref_off), R, ref_boxes.shape[1], int(ncls), float(dist_th), int(max_boxes), _ptr(class_range),
             _ptr(origin), _view4(view), _ptr(out["match_ref"]), _ptr(out["match_iou"]), _ptr(out["cls_count"]),
             _ptr(out["cls_quality"]), _ptr(out["cls_cons"]), _ptr(status), _stream())
    st = int(status.item())
    if st & MATCH_TOO_MANY_BOXES:
        raise AssertionError(f"Error: Only <= {int(max_boxes)} boxes per sample allowed!")      # the devkit's message
    if st & MATCH_CLASS_TOO_LARGE:
        raise lib.Al3dError("match_boxes: one class of one frame holds more than 512 predictions or 1024 reference boxes")
    if st:
        raise lib.Al3dError(f"match_boxes: ref_off is not ascending inside [0, {R}] (status {st})")
    return out


# ---------------------------------------------------------------- rotated box IoU and NMS (al3d_box_iou_* / al3d_nms_boxes_*)
BOX_CONVENTION = {"det3d": 0, "heading": 1}                      # AL3D_BOX_*
BOX_LAYOUT = {"xyzwlhr": 0, "xyxyr": 1}                          # AL3D_BOX_ROWS_*
IOU_HEIGHT = {"_bev": 0, "3d": 1, "3d_kitti": 2}                 # name suffix -> AL3D_IOU_H_*
# metric name -> (AL3D_IOU_* formula, height rule): iou_bev, iou3d, iou3d_kitti, overlap_bev, over_a3d, ...
IOU_METRIC = {k + h: (v, hv) for k, v in (("overlap", 0), ("iou", 1), ("over_a", 2), ("over_b", 3))
              for h, hv in IOU_HEIGHT.items()}
NMS_MODE = {"rotated": 0, "normal": 1}                           # AL3D_NMS_*
BOX_IOU_TILE_ROWS, BOX_IOU_TILE_COLS, BOX_IOU_ROWS_MAX = 16, 64, 128
NMS_MAX_CANDIDATES = 4096
IOU_BAD_OFFSETS = 1


def _enum(table, key, what):
    if key not in table:
        raise lib.Al3dError(f"{what}: {key!r} is not one of {sorted(table)}")
    return table[key]


def _box_rows(t, name, layout, rot_col):
    t = _dev(t, torch.float32, name)
    need = 5 if layout == "xyxyr" else 7
    if t.dim() != 2 or t.shape[1] < need:
        raise lib.Al3dError(f"{name}: [n, >={need}] float32 rows expected for layout {layout!r}")
    if layout != "xyxyr" and not 6 <= int(rot_col) < t.shape[1]:
        raise lib.Al3dError(f"{name}: rot_col {rot_col} outside [6, {t.shape[1]})")
    return t


def box_iou_matrix(a, b, metric="iou_bev", convention="det3d", rot_col=6, layout="xyzwlhr", rot_col_b=None, launch=None):
    """``a [N,D]``, ``b [M,D']`` f32 device rows -> ``[N, M]`` f32 (``al3d_box_iou_matrix_f32`` in include/al3d.h).

    ``metric``: ``iou`` / ``overlap`` / ``over_a`` / ``over_b`` + ``_bev`` (footprints), ``3d`` (height z +- h/2, volumes) or
    ``3d_kitti`` (height [z - h, z]); ``convention``: ``det3d`` (rotation_2d) or ``heading`` (OpenPCDet); ``layout``:
    ``xyzwlhr`` (angle in ``rot_col`` / ``rot_col_b``) or ``xyxyr``.  ``launch = (tile_rows, threads, reject)`` is for the
    tests and the benchmark."""
    m, h = _enum(IOU_METRIC, metric, "box_iou_matrix: metric")
    conv, lay = _enum(BOX_CONVENTION, convention, "box_iou_matrix: convention"), _enum(BOX_LAYOUT, layout, "box_iou_matrix: layout")
    rot_b = rot_col if rot_col_b is None else rot_col_b
    a, b = _box_rows(a, "a", layout, rot_col), _box_rows(b, "b", layout, rot_b)
    if lay == 1 and h:
        raise lib.Al3dError("box_iou_matrix: [x1, y1, x2, y2, r] rows have no height; use a _bev metric")
    n, mm = a.shape[0], b.shape[0]
    out = torch.empty((n, mm), dtype=torch.float32, device=a.device)
    args = (_ptr(a) if n else None, n, a.shape[1], int(rot_col), _ptr(b) if mm else None, mm, b.shape[1], int(rot_b), lay, conv, m,
            h, _ptr(out) if n * mm else None)
    if launch is None:
        lib.call("al3d_box_iou_matrix_f32", *args, _stream())
    else:
        lib.call("al3d_box_iou_matrix_launch_f32", *args, int(launch[0]), int(launch[1]), int(launch[2]), _stream())
    return out


def box_iou_best(boxes, labels, counts, ref_boxes, ref_labels, ref_off, metric="iou3d", convention="det3d", rot_col=None,
                 ref_rot_col=6, same_class=False, launch=None):
    """The best IoU of every detection against its frame's reference boxes (``al3d_box_iou_best_f32``), on the raw NMS
    buffers: ``boxes [B,nt,post,D]`` f32, ``labels [B,nt,post]`` i32, ``counts [B,nt]`` i32; ``ref_boxes [R,>=7]`` f32,
    ``ref_labels [R]`` i32, ``ref_off [B+1]`` i32 (``FrameRefs.batch``).  ``rot_col`` defaults to the last column, as the
    9-column NMS buffers keep the angle.  -> ``(best_iou [B,nt,post] f32, best_ref [B,nt,post] i32)``; the row maximum of
    ``box_iou_matrix`` per frame with the lowest row among equal maxima, 0 / -1 where there is none.  Reads the status word
    back (one small D2H).  ``launch = (chunk, ref_tile, threads, reject)`` is for the tests and the benchmark."""
    m, h = _enum(IOU_METRIC, metric, "box_iou_best: metric")
    conv = _enum(BOX_CONVENTION, convention, "box_iou_best: convention")
    boxes = _dev(boxes, torch.float32, "boxes")
    labels = _dev(labels, torch.int32, "labels")
    counts = _dev(counts, torch.int32, "counts")
    ref_labels = _dev(ref_labels, torch.int32, "ref_labels")
    ref_off = _dev(ref_off, torch.int32, "ref_off")
    if boxes.dim() != 4 or labels.shape != boxes.shape[:3] or counts.shape != boxes.shape[:2] or boxes.shape[3] < 7:
        raise lib.Al3dError("box_iou_best: boxes [B,nt,post,>=7], labels [B,nt,post], counts [B,nt] expected")
    B, nt, post, bd = boxes.shape
    rot_col = bd - 1 if rot_col is None else int(rot_col)
    if not 6 <= rot_col < bd:
        raise lib.Al3dError(f"box_iou_best: rot_col {rot_col} outside [6, {bd})")
    ref_boxes = _box_rows(ref_boxes, "ref_boxes", "xyzwlhr", ref_rot_col)
    R = ref_boxes.shape[0]
    if ref_labels.shape != (R,) or ref_off.shape != (B + 1,):
        raise lib.Al3dError("box_iou_best: ref_boxes [R,>=7], ref_labels [R], ref_off [B+1] expected")
    dev = boxes.device
    best_iou = torch.empty((B, nt, post), dtype=torch.float32, device=dev)
    best_ref = torch.empty((B, nt, post), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    args = (_ptr(boxes), _ptr(labels), _ptr(counts), B, nt, post, bd, rot_col, _ptr(ref_boxes) if R else None,
            _ptr(ref_labels) if R else None, _ptr(ref_off), R, ref_boxes.shape[1], int(ref_rot_col), conv, m, h,
            1 if same_class else 0, _ptr(best_iou), _ptr(best_ref), _ptr(status))
    if launch is None:
        lib.call("al3d_box_iou_best_f32", *args, _stream())
    else:
        lib.call("al3d_box_iou_best_launch_f32", *args, *(int(v) for v in launch), _stream())
    if int(status.item()) & IOU_BAD_OFFSETS:
        raise lib.Al3dError(f"box_iou_best: ref_off is not ascending inside [0, {R}]")
    return best_iou, best_ref


def nms_boxes(boxes, scores, thresh, pre_max=None, post_max=None, mode="rotated", convention="heading", rot_col=6,
              layout="xyzwlhr", launch=None):
    """Greedy NMS on device rows (``al3d_nms_boxes_f32``): ``boxes [N,D]``, ``scores [N]`` f32 -> ``keep [k]`` i64, indices into
    the input in descending score order (NaN scores last, equal scores by the lower index).  A box falls when its IoU with an
    earlier kept one is ``> thresh``; ``mode="normal"`` compares the axis-aligned boxes.  At most 4096 candidates after
    ``pre_max``.  Reads the count back (one small D2H).  ``launch = (sort_threads, mask_threads, reject)`` is for the tests."""
    mode_i = _enum(NMS_MODE, mode, "nms_boxes: mode")
    conv, lay = _enum(BOX_CONVENTION, convention, "nms_boxes: convention"), _enum(BOX_LAYOUT, layout, "nms_boxes: layout")
    boxes = _box_rows(boxes, "boxes", layout, rot_col)
    scores = _dev(scores, torch.float32, "scores")
    n = boxes.shape[0]
    if scores.shape != (n,):
        raise lib.Al3dError("nms_boxes: boxes [N,D] and scores [N] expected")
    pre = 0 if pre_max is None else int(pre_max)
    post = 0 if post_max is None else int(post_max)
    cand = min(n, pre) if pre > 0 else n
    if cand > NMS_MAX_CANDIDATES:
        raise lib.Al3dError(f"nms_boxes: {cand} candidates after pre_max, at most {NMS_MAX_CANDIDATES}")
    cap = min(cand, post) if post > 0 else cand
    dev = boxes.device
    keep = torch.empty((max(cap, 1),), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.load().al3d_nms_boxes_workspace_bytes(n),), dtype=torch.uint8, device=dev)
    args = (_ptr(boxes) if n else None, _ptr(scores) if n else None, n, boxes.shape[1], int(rot_col), lay, conv, mode_i,
            float(thresh), pre, post, _ptr(keep), cap, _ptr(count), _ptr(ws))
    if launch is None:
        lib.call("al3d_nms_boxes_f32", *args, _stream())
    else:
        lib.call("al3d_nms_boxes_launch_f32", *args, *(int(v) for v in launch), _stream())
    return keep[:int(count.item())].long()


EST_MAX_BOXES, EST_MAX_CLASSES, EST_BAD_OFFSETS, EST_BAD_LABEL = 1024, 32, 1, 2      # AL3D_EST_* of include/al3d.h


def estimator_status_check(status):
    """Raise for the AL3D_EST_* bits of a status word that is on the host already."""
    st = int(status)
    if st & EST_BAD_OFFSETS:
        raise lib.Al3dError("estimate_boxes: point_offsets is not ascending inside [0, number of points]")
    if st & EST_BAD_LABEL:
        raise lib.Al3dError("estimate_boxes: a detection's label lies outside [0, num_classes)")
    if st:
        raise lib.Al3dError(f"estimate_boxes: status {st}")


def estimate_boxes(boxes, labels, counts, points, point_offsets, weights, num_classes, rot_col=6, out=None, check=True):
    """The box-wise IoU estimator on the raw NMS buffers (``al3d_estimator_f32`` in include/al3d.h; reference
    estimator.py:92-105,155-274).

    ``boxes [B,nt,post,D]`` f32, ``labels [B,nt,post]`` i32, ``counts [B,nt]`` i32; ``points [P,F]`` f32 with the frames
    back to back and ``point_offsets [B+1]`` i64; ``weights``: the folded, packed network (``models.estimator``).  Returns
    ``dict(boxes, scores, labels, counts)`` -- the boxes that hold a point, compacted per (frame, task), scored with the
    predicted IoU -- plus ``npts [B,nt,post]`` i32 and ``pooled [B,nt,post,128]`` f32 (views of the workspace, per INPUT
    slot) and ``status`` (device i32).  ``out``: buffers to write instead of fresh zeroed ones.  ``check=True`` reads the
    status word back (one small D2H) and raises ``Al3dError``; with ``check=False`` nothing synchronises and the caller
    hands ``status`` to ``estimator_status_check`` when it next reads from the device."""
    boxes = _dev(boxes, torch.float32, "boxes")
    labels = _dev(labels, torch.int32, "labels")
    counts = _dev(counts, torch.int32, "counts")
    points = _dev(points, torch.float32, "points")
    point_offsets = _dev(point_offsets, torch.int64, "point_offsets")
    weights = _dev(weights, torch.float32, "weights")
    if boxes.dim() != 4 or labels.shape != boxes.shape[:3] or counts.shape != boxes.shape[:2]:
        raise lib.Al3dError("estimate_boxes: boxes [B,nt,post,D], labels [B,nt,post], counts [B,nt] expected")
    B, nt, post, bd = boxes.shape
    if points.dim() != 2 or point_offsets.shape != (B + 1,) or weights.dim() != 1:
        raise lib.Al3dError("estimate_boxes: points [P,F], point_offsets [B+1], weights [n] expected")
    dev = boxes.device
    if out is None:
        out = dict(boxes=torch.zeros_like(boxes), scores=torch.zeros((B, nt, post), dtype=torch.float32, device=dev),
                   labels=torch.zeros_like(labels), counts=torch.zeros_like(counts))
    ws_bytes = lib.load().al3d_estimator_workspace_bytes(B, nt, post)
    ws = torch.empty((max(ws_bytes, 512),), dtype=torch.uint8, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    lib.call("al3d_estimator_f32", _ptr(boxes), _ptr(labels), _ptr(counts), B, nt, post, bd, int(rot_col),
             _ptr(points) if points.shape[0] else None, _ptr(point_offsets), points.shape[0], points.shape[1],
             _ptr(weights), weights.numel(), int(num_classes), _ptr(out["boxes"]), _ptr(out["scores"]), _ptr(out["labels"]),
             _ptr(out["counts"]), _ptr(ws), _ptr(status), _stream())
    slots = B * nt * post
    a0 = (-ws.data_ptr()) % 256                      # the entry aligns the workspace to 256 bytes itself
    a1 = a0 + (slots * 4 + 255) // 256 * 256
    res = dict(out)
    res["npts"] = ws[a0:a0 + slots * 4].view(torch.int32).view(B, nt, post)
    res["pooled"] = ws[a1:a1 + slots * 512].view(torch.float32).view(B, nt, post, 128)
    res["status"] = status
    if check:
        estimator_status_check(status.item())
    return res


def points_view_(points, view):
    """In place on the xyz columns of ``points [P,F]``: ``view = (flip_x, flip_y, rot, scale)`` -- y negated if ``flip_x``,
    x negated if ``flip_y`` (det3d's naming), then the rotation about z, then the scaling (preprocess.py:787-854)."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32 or \
            points.dim() != 2 or not points.is_contiguous():
        raise lib.Al3dError("points_view_: expected a contiguous [P,F] float32 device tensor (no CPU fallback)")
    fx, fy, rot, scale = view
    lib.call("al3d_points_view_f32", _ptr(points), points.shape[0], points.shape[1], 1 if fx else 0, 1 if fy else 0,
             float(rot), float(scale), _stream())
    return points


def mask_map_(D, keep):
    """In place: D[i,j] = -inf unless keep[i] and keep[j] (keep: uint8 [n])."""
    D = _dev(D, torch.float32, "D")
    keep = _dev(keep, torch.uint8, "keep")
    lib.call("al3d_mask_map_f32", _ptr(D), D.shape[0], _ptr(keep), _stream())
    return D


def scale_rows(feats, w, widx=None):
    feats = _dev(feats, torch.float32, "feats")
    w = _dev(w, torch.float32, "w")
    widx = _dev(widx, torch.int64, "widx")
    n, c = feats.shape
    out = torch.empty_like(feats)
    lib.call("al3d_scale_rows_f32", _ptr(feats), _ptr(w), _ptr(widx), n, c, _ptr(out), _stream())
    return out


def minmax_norm(x):
    x = _dev(x, torch.float32, "x")
    out = torch.empty_like(x)
    lib.call("al3d_minmax_norm_f32", _ptr(x), x.numel(), _ptr(out), _stream())
    return out


def argsort_desc(x):
    """torch.argsort(-x) semantics: descending, NaN last, ties by ascending index."""
    x = _dev(x, torch.float32, "x")
    n = x.numel()
    out = torch.empty((n,), dtype=torch.int64, device=x.device)
    ws = torch.empty(max(8, lib.load().al3d_argsort_workspace_bytes(n)), dtype=torch.uint8, device=x.device)
    lib.call("al3d_argsort_desc_f32", _ptr(x), n, _ptr(out), _ptr(ws), _stream())
    return out


def greedy_kcenter(D, seeded, first, box_cost, cost_f, start_cost, budget_int, seed_map=None,
                   check_seeded=False, cap=None):
    """Run the whole pick loop on device.  Returns (status, picks[list[int]])."""
    if D.dtype not in (torch.float64, torch.float32):
        raise lib.Al3dError(f"greedy_kcenter: unsupported map dtype {D.dtype}")
    D = _dev(D, D.dtype, "D")
    seed_map = D if seed_map is None else _dev(seed_map, D.dtype, "seed_map")
    n = D.shape[0]
    dev = D.device
    seeded_t = torch.as_tensor(list(seeded), dtype=torch.int64, device=dev)
    if seeded_t.numel() and (int(seeded_t.min()) < 0 or int(seeded_t.max()) >= n):
        raise lib.Al3dError("greedy_kcenter: seeded index outside the pool")
    box_cost = _dev(box_cost, torch.float64, "box_cost")
    cap = n + 1 if cap is None else int(cap)
    out_idx = torch.empty(cap, dtype=torch.int64, device=dev)
    meta = torch.zeros(2, dtype=torch.int64, device=dev)
    esz = D.element_size()
    ws = torch.empty(lib.load().al3d_greedy_workspace_bytes(n, esz), dtype=torch.uint8, device=dev)
    fn = "al3d_greedy_kcenter_f64" if D.dtype == torch.float64 else "al3d_greedy_kcenter_f32"
    lib.call(fn, _ptr(D), _ptr(seed_map), n, _ptr(seeded_t) if seeded_t.numel() else None,
             int(seeded_t.numel()), int(first), _ptr(box_cost), float(cost_f), float(start_cost),
             float(budget_int), 1 if check_seeded else 0, _ptr(out_idx), cap, _ptr(meta), _ptr(ws),
             _stream())
    cnt, status = meta.tolist()
    return int(status), out_idx[:cnt].tolist()


# AL3D_PIB_* of include/al3d.h
PIB_BAD_POINT_OFF, PIB_BAD_BOX_OFF, PIB_FRAME_TOO_LARGE, PIB_BAD_WORKSPACE, PIB_BAD_ROWS = 1, 2, 4, 8, 16
PIB_GROUPS, PIB_THREADS, PIB_TILE = 32, 256, 64


def pib_status_check(status, who="points_in_boxes"):
    """Raise for the AL3D_PIB_* bits of a status word that is on the host already."""
    st = int(status)
    if st & PIB_BAD_POINT_OFF:
        raise lib.Al3dError(f"{who}: point_off is not ascending inside [0, number of points]")
    if st & PIB_BAD_BOX_OFF:
        raise lib.Al3dError(f"{who}: box_off is not ascending inside [0, number of boxes]")
    if st & PIB_FRAME_TOO_LARGE:
        raise lib.Al3dError(f"{who}: a frame has 2^31 points or more")
    if st:
        raise lib.Al3dError(f"{who}: status {st} (workspace or offsets do not belong to this call)")


def _pib_planes(boxes, planes, device):
    """``[R, 6, 4]`` device planes: the caller's, or ``detector_ops.box_planes`` of host boxes (one small upload)."""
    if planes is None:
        from .detector_ops import box_planes
        if isinstance(boxes, torch.Tensor):
            boxes = boxes.detach().cpu().numpy()
        planes = torch.from_numpy(box_planes(boxes)).to(device)
    planes = _dev(planes, torch.float32, "planes")
    if planes.dim() != 3 or planes.shape[1:] != (6, 4):
        raise lib.Al3dError("points_in_boxes: planes [R, 6, 4] expected")
    return planes


def points_in_boxes_count(points, point_off, planes, box_off, launch=None):
    """``al3d_points_in_boxes_count_f32``: -> ``(box_count [R] i32, workspace, status)`` on the device, nothing read back.
    ``launch = (groups, threads, tile)`` is for the tests and the benchmark."""
    points = _dev(points, torch.float32, "points")
    point_off = _dev(point_off, torch.int64, "point_off")
    box_off = _dev(box_off, torch.int32, "box_off")
    planes = _pib_planes(None, planes, points.device)
    if points.dim() != 2 or points.shape[1] < 3 or point_off.dim() != 1 or point_off.numel() < 1 or \
            box_off.shape != point_off.shape:
        raise lib.Al3dError("points_in_boxes: points [P, >= 3], point_off [B+1] i64, box_off [B+1] i32 expected")
    g, t, tile = (PIB_GROUPS, PIB_THREADS, PIB_TILE) if launch is None else (int(v) for v in launch)
    P, F, B, R = points.shape[0], points.shape[1], point_off.numel() - 1, planes.shape[0]
    dev = points.device
    nbytes = int(lib.load().al3d_points_in_boxes_workspace_bytes(R, g, t))
    if nbytes < 0:
        raise lib.Al3dError(f"points_in_boxes: bad launch shape {(g, t, tile)} or box count {R}")
    ws = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=dev)
    counts = torch.empty((R,), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    lib.call("al3d_points_in_boxes_count_launch_f32", _ptr(points) if P else None, P, F, _ptr(point_off), B,
             _ptr(planes) if R else None, _ptr(box_off), R, _ptr(counts) if R else None, _ptr(ws), _ptr(status), g, t, tile,
             _stream())
    return counts, ws, status


def points_in_boxes_gather(points, point_off, planes, box_off, out_off, centres, workspace, total, num_features, launch=None):
    """``al3d_points_in_boxes_gather_f32`` after ``points_in_boxes_count`` with the same ``launch`` groups and threads:
    -> ``(rows [total, num_features] f32, index [total] i64, status)`` on the device."""
    points = _dev(points, torch.float32, "points")
    point_off = _dev(point_off, torch.int64, "point_off")
    box_off = _dev(box_off, torch.int32, "box_off")
    planes = _pib_planes(None, planes, points.device)
    out_off = _dev(out_off, torch.int64, "out_off")
    centres = _dev(centres, torch.float32, "centres")
    P, F, B, R = points.shape[0], points.shape[1], point_off.numel() - 1, planes.shape[0]
    if out_off.shape != (R + 1,) or centres.shape != (R, 3) or not 3 <= int(num_features) <= F:
        raise lib.Al3dError("points_in_boxes: out_off [R+1], centres [R, 3] and 3 <= num_features <= F expected")
    g, t, tile = (PIB_GROUPS, PIB_THREADS, PIB_TILE) if launch is None else (int(v) for v in launch)
    dev = points.device
    T = int(total)
    rows = torch.empty((T, int(num_features)), dtype=torch.float32, device=dev)
    index = torch.empty((T,), dtype=torch.int64, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    lib.call("al3d_points_in_boxes_gather_launch_f32", _ptr(points) if P else None, P, F, _ptr(point_off), B,
             _ptr(planes) if R else None, _ptr(box_off), R, _ptr(out_off), _ptr(centres) if R else None, _ptr(workspace),
             _ptr(rows) if T else None, int(num_features), _ptr(index) if T else None, T, _ptr(status), g, t, tile, _stream())
    return rows, index, status


def points_in_boxes(points, point_off, boxes, box_off, num_features, planes=None, launch=None, check=True):
    """Every box's points, compacted (the device half of ``create_groundtruth_database``; include/al3d.h, "points in boxes").

    ``points [P, F]`` f32 with the frames back to back, ``point_off [B+1]`` i64, ``boxes [R, >= 7]`` f32 (host numpy or a
    tensor: centre, sizes, ..., the angle LAST) with the frames' boxes back to back, ``box_off [B+1]`` i32.  Returns
    ``(rows [T, num_features] f32, index [T] i64, counts [R] i32, offsets [R+1] i64)``: box r's rows are
    ``rows[offsets[r]:offsets[r+1]]``, its points in ascending point index with xyz minus the box centre, ``index`` the row
    of ``points`` each came from.  Flow: count, ONE host read (the total, with the count's status word), gather; with
    ``check=True`` the gather's status word is read back afterwards (it can only be set by a workspace or offsets that are
    not this call's own).  ``planes`` overrides ``detector_ops.box_planes(boxes)``; ``launch = (groups, threads, tile)`` is
    for the tests and the benchmark."""
    points = _dev(points, torch.float32, "points")
    dev = points.device
    if isinstance(boxes, torch.Tensor):
        centres = boxes[:, :3].to(device=dev, dtype=torch.float32).contiguous()
    else:
        import numpy as np
        centres = torch.from_numpy(np.ascontiguousarray(np.asarray(boxes)[:, :3], dtype=np.float32)).to(dev)
    planes = _pib_planes(boxes, planes, dev)
    R = planes.shape[0]
    if centres.shape != (R, 3):
        raise lib.Al3dError("points_in_boxes: boxes [R, >= 7] and planes [R, 6, 4] expected")
    counts, ws, st_count = points_in_boxes_count(points, point_off, planes, box_off, launch)
    offsets = torch.zeros((R + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    total, st = torch.stack([offsets[R], st_count[0].to(torch.int64)]).tolist()       # the one host read
    pib_status_check(st)
    rows, index, st_gather = points_in_boxes_gather(points, point_off, planes, box_off, offsets, centres, ws, total,
                                                    num_features, launch)
    if check:
        pib_status_check(st_gather.item())
    return rows, index, counts, offsets


def points_in_boxes_mask(points, planes, launch=None):
    """``al3d_points_in_boxes_mask_u8``: ``points [P, F]`` f32, ``planes [R, 6, 4]`` f32 -> ``[P, R]`` uint8, the
    ``points_in_rbbox`` matrix of one frame.  ``launch = (threads, tile)``."""
    points = _dev(points, torch.float32, "points")
    planes = _pib_planes(None, planes, points.device)
    if points.dim() != 2 or points.shape[1] < 3:
        raise lib.Al3dError("points_in_boxes_mask: points [P, >= 3] expected")
    P, F, R = points.shape[0], points.shape[1], planes.shape[0]
    out = torch.empty((P, R), dtype=torch.uint8, device=points.device)
    args = (_ptr(points) if P else None, P, F, _ptr(planes) if R else None, R, _ptr(out) if P * R else None)
    if launch is None:
        lib.call("al3d_points_in_boxes_mask_u8", *args, _stream())
    else:
        lib.call("al3d_points_in_boxes_mask_launch_u8", *args, *(int(v) for v in launch), _stream())
    return out
