"""Train-mode augmentation (reference ``det3d/core/sampler/preprocess.py`` and the train branch of
``det3d/datasets/pipelines/preprocess.py:57-256``): boxes are host numpy, points are device tensors.

The draws are numpy's, made with the reference's own calls in its order, so a seeded ``np.random`` is consumed exactly as
the reference consumes it.  The per-box noise search runs in ``al3d_noise_per_box_f32`` and every step that touches a point
in ONE launch of ``al3d_augment_points_f32`` (csrc/augment.hip); the boxes, a few tens per frame, follow the reference's
numpy lines on the host.  The box columns are the reference's, literally: ``noise_per_object_v3_`` reads column 6 as the angle
and adds the rotation noise to column 6 (the ``vx`` column of a 9-column nuScenes box), the sampler and the global steps use
``[:, -1]``.

``augment_batch`` is what ``Preprocess(mode="train")`` and ``FileSweepLoader(train_cfg=...)`` call.  For a batch it draws in
two rounds -- sampling and the per-object noises of every frame, then flips, rotation, scale and shuffle of every frame -- so a
batch of one frame draws in the reference's order.  Host reads: ``selected`` (with the kept counts when
``remove_points_after_sample`` can drop something), once per batch, before the shuffle is drawn.
"""
import numpy as np
import torch

from .. import lib

AUG_GROUPS, AUG_THREADS, AUG_TILE, AUG_NOISE_TILE = 32, 256, 64, 4
AUG_MAX_BOXES, AUG_MAX_TRIES = 1024, 256
AUG_STATUS = {1: "point_off is not ascending inside [0, number of points]", 2: "box_off is not ascending inside [0, number of boxes]",
              4: "a frame has 2^31 points or more", 8: "the workspace belongs to another call or launch shape",
              16: "a destination row lies outside its frame", 32: f"a frame has more than {AUG_MAX_BOXES} boxes",
              64: f"num_try outside [1, {AUG_MAX_TRIES}]", 128: "sampled_off outside its frame", 256: "selected outside [-1, num_try)"}


def aug_status_check(status, who="augment"):
    st = int(status)
    if st:
        raise lib.Al3dError(f"{who}: " + "; ".join(v for k, v in AUG_STATUS.items() if st & k))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _up(a, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


# ---- host geometry, the reference's own numpy calls ------------------------------------------------------------------------
def box2d_to_corner(boxes):
    """``box2d_to_corner_jit`` (box_np_ops.py:503-521): ``[N, 5]`` (x, y, w, l, angle) -> ``[N, 4, 2]``, in the boxes' dtype."""
    boxes = np.asarray(boxes)
    n = boxes.shape[0]
    norm = np.zeros((4, 2), dtype=boxes.dtype)
    norm[1, 1] = 1.0
    norm[2] = 1.0
    norm[3, 0] = 1.0
    norm -= np.array([0.5, 0.5], dtype=boxes.dtype)
    corners = boxes.reshape(n, 1, 5)[:, :, 2:4] * norm.reshape(1, 4, 2)
    rot = np.zeros((2, 2), dtype=boxes.dtype)
    out = np.zeros((n, 4, 2), dtype=boxes.dtype)
    for i in range(n):
        s, c = np.sin(boxes[i, -1]), np.cos(boxes[i, -1])
        rot[0, 0], rot[0, 1], rot[1, 0], rot[1, 1] = c, -s, s, c
        out[i] = corners[i] @ rot + boxes[i, :2]
    return out


def _corners_nd(dims, origin):
    ndim = int(dims.shape[1])
    norm = np.stack(np.unravel_index(np.arange(2 ** ndim), [2] * ndim), axis=1).astype(dims.dtype)
    norm = norm[[0, 1, 3, 2]] if ndim == 2 else norm[[0, 1, 3, 2, 4, 5, 7, 6]]
    norm = norm - np.array(origin, dtype=dims.dtype)
    return dims.reshape([-1, 1, ndim]) * norm.reshape([1, 2 ** ndim, ndim])


def center_to_corner_box2d(centers, dims, angles=None, origin=0.5):
    """box_np_ops.py:479-499 with ``corners_nd`` (:269-299) and ``rotation_2d`` (:421-434)."""
    corners = _corners_nd(dims, origin)
    if angles is not None:
        s, c = np.sin(angles), np.cos(angles)
        corners = np.einsum("aij,jka->aik", corners, np.stack([[c, -s], [s, c]]))
    corners += centers.reshape([-1, 1, 2])
    return corners


def rotation_points_single_angle(points, angle):
    """box_np_ops.py:396-418, ``axis=2``."""
    s, c = np.sin(angle), np.cos(angle)
    return points @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=points.dtype)


def box_collision_test(boxes, qboxes, clockwise=True):
    """``box_collision_test`` (sampler/preprocess.py:876-959) vectorised: ``[N, 4, 2]`` x ``[K, 4, 2]`` corners ->
    ``[N, K]`` bool.  The stand-up rejection (``> 0``) first; the 4 x 4 strict segment test and the two containment tests
    (``cross >= 0`` ends a test) only on the surviving pairs, in the corners' own dtype."""
    boxes, qboxes = np.asarray(boxes), np.asarray(qboxes)
    N, K = boxes.shape[0], qboxes.shape[0]
    ret = np.zeros((N, K), dtype=np.bool_)
    if N == 0 or K == 0:
        return ret
    bs = np.concatenate([boxes.min(1), boxes.max(1)], axis=1)
    qs = np.concatenate([qboxes.min(1), qboxes.max(1)], axis=1)
    iw = np.minimum(bs[:, None, 2], qs[None, :, 2]) - np.maximum(bs[:, None, 0], qs[None, :, 0])
    ih = np.minimum(bs[:, None, 3], qs[None, :, 3]) - np.maximum(bs[:, None, 1], qs[None, :, 1])
    ii, jj = np.nonzero((iw > 0) & (ih > 0))
    if len(ii) == 0:
        return ret
    nxt = [1, 2, 3, 0]
    b, q = boxes[ii], qboxes[jj]                                           # [M, 4, 2]
    A, B = b[:, :, None, :], b[:, nxt][:, :, None, :]                       # [M, 4(k), 1, 2]
    C, D = q[:, None, :, :], q[:, nxt][:, None, :, :]                       # [M, 1, 4(l), 2]
    acd = (D[..., 1] - A[..., 1]) * (C[..., 0] - A[..., 0]) > (C[..., 1] - A[..., 1]) * (D[..., 0] - A[..., 0])
    bcd = (D[..., 1] - B[..., 1]) * (C[..., 0] - B[..., 0]) > (C[..., 1] - B[..., 1]) * (D[..., 0] - B[..., 0])
    abc = (C[..., 1] - A[..., 1]) * (B[..., 0] - A[..., 0]) > (B[..., 1] - A[..., 1]) * (C[..., 0] - A[..., 0])
    abd = (D[..., 1] - A[..., 1]) * (B[..., 0] - A[..., 0]) > (B[..., 1] - A[..., 1]) * (D[..., 0] - A[..., 0])
    hit = ((acd != bcd) & (abc != abd)).any(axis=(1, 2))

    def holds(outer, inner):                                               # every corner of `inner` strictly inside `outer`
        vec = outer - outer[:, nxt]
        if clockwise:
            vec = -vec
        cross = vec[:, :, None, 1] * (outer[:, :, None, 0] - inner[:, None, :, 0])
        cross = cross - vec[:, :, None, 0] * (outer[:, :, None, 1] - inner[:, None, :, 1])
        return ~(cross >= 0).any(axis=(1, 2))

    over = holds(b, q)
    over = over | (~over & holds(q, b))
    ret[ii, jj] = hit | over
    return ret


def filter_gt_box_outside_range(gt_boxes, limit_range):
    """sampler/preprocess.py:133-147: a box stays when any BEV corner lies strictly inside the range rectangle."""
    gt_boxes = np.asarray(gt_boxes)
    bv = center_to_corner_box2d(gt_boxes[:, [0, 1]], gt_boxes[:, [3, 4]], gt_boxes[:, -1])
    rng = np.asarray(limit_range)[np.newaxis, ...]
    poly = center_to_corner_box2d(rng[..., :2], rng[..., 2:] - rng[..., :2], origin=0.0)      # minmax_to_corner_2d
    pts = bv.reshape(-1, 2)
    vec1 = poly - poly[:, [3, 0, 1, 2], :]
    cross = vec1[None, 0, :, 1] * (poly[None, 0, :, 0] - pts[:, None, 0])
    cross = cross - vec1[None, 0, :, 0] * (poly[None, 0, :, 1] - pts[:, None, 1])
    inside = ~(cross >= 0).any(axis=1)
    return np.any(inside.reshape(-1, 4), axis=1)


# ---- device entries --------------------------------------------------------------------------------------------------------
def _launch(launch, noise=False):
    if launch is None:
        return AUG_GROUPS, AUG_THREADS, AUG_NOISE_TILE if noise else AUG_TILE
    return tuple(int(v) for v in launch)


def noise_per_box_device(corners, centres, valid, rot_cos, rot_sin, loc, box_off, launch=None):
    """``al3d_noise_per_box_f32`` on device tensors -> ``(selected [R] i32, status [1] i32)``, nothing read back."""
    R, T, B = corners.shape[0], rot_cos.shape[1] if rot_cos.dim() == 2 else 0, box_off.numel() - 1
    dev = box_off.device
    selected = torch.full((R,), -1, dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    g, t, tile = _launch(launch, noise=True)
    lib.call("al3d_noise_per_box_launch_f32", _ptr(corners), _ptr(centres), _ptr(valid), _ptr(rot_cos), _ptr(rot_sin), _ptr(loc),
             _ptr(box_off), B, R, T, _ptr(selected), _ptr(status), g, t, tile, _stream())
    return selected, status


def augment_points_count(points, point_off, sampled_off, drop_planes, drop_off, launch=None):
    """``al3d_augment_points_count_f32`` -> ``(drop_mask [P] u8, kept [B] i32, workspace, status)`` on the device."""
    P, F, B, R = points.shape[0], points.shape[1], point_off.numel() - 1, drop_planes.shape[0]
    dev = points.device
    g, t, tile = _launch(launch)
    nbytes = int(lib.load().al3d_augment_points_workspace_bytes(B, g, t))
    if nbytes < 0:
        raise lib.Al3dError(f"augment_points_count: bad launch shape {(g, t, tile)} or batch {B}")
    ws = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=dev)
    drop_mask = torch.zeros((P,), dtype=torch.uint8, device=dev)
    kept = torch.zeros((B,), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    lib.call("al3d_augment_points_count_launch_f32", _ptr(points), P, F, _ptr(point_off), sampled_off.data_ptr(), B,
             _ptr(drop_planes), drop_off.data_ptr(), R, _ptr(drop_mask), kept.data_ptr(), ws.data_ptr(), status.data_ptr(),
             g, t, tile, _stream())
    return drop_mask, kept, ws, status


def augment_points(points, point_off, out_off, out_rows, global_xf, *, drop_mask=None, workspace=None, planes=None, box_off=None,
                   valid=None, centres=None, rot_cos=None, rot_sin=None, loc=None, selected=None, flip=None, symmetry=False,
                   rows=None, want_owner=False, out=None, launch=None):
    """``al3d_augment_points_f32`` -> ``(out [out_rows, F] f32, owner [P] i32 or None, status)`` on the device."""
    P, F, B = points.shape[0], points.shape[1], point_off.numel() - 1
    R = 0 if planes is None else planes.shape[0]
    T = 0 if rot_cos is None or rot_cos.dim() != 2 else rot_cos.shape[1]
    dev = points.device
    g, t, tile = _launch(launch)
    if out is None:
        out = torch.empty((int(out_rows), F), dtype=torch.float32, device=dev)
    owner = torch.full((P,), -1, dtype=torch.int32, device=dev) if want_owner else None
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    lib.call("al3d_augment_points_launch_f32", _ptr(points), P, F, _ptr(point_off), B,
             None if drop_mask is None else drop_mask.data_ptr(), None if workspace is None else workspace.data_ptr(),
             _ptr(planes) if R else None, box_off.data_ptr() if R else None, R, _ptr(valid) if R else None,
             _ptr(centres) if R else None, _ptr(rot_cos) if R else None, _ptr(rot_sin) if R else None,
             _ptr(loc) if R else None, _ptr(selected) if R else None, T, None if flip is None else flip.data_ptr(),
             global_xf.data_ptr(), 1 if symmetry else 0, out_off.data_ptr(), None if rows is None else _ptr(rows), _ptr(out),
             int(out_rows), None if owner is None else _ptr(owner), status.data_ptr(), g, t, tile, _stream())
    return out, owner, status


def _one_frame_pass(points, flip=(False, False), cos=1.0, sin=0.0, scale=1.0):
    """A global step alone on one cloud, in place (what the stand-alone mirrors below launch)."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32 or not points.is_contiguous():
        raise lib.Al3dError("augment: points must be a contiguous float32 device tensor (no CPU fallback)")
    dev, n = points.device, points.shape[0]
    off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    xf = torch.tensor([[np.float32(cos), np.float32(sin), np.float32(scale)]], dtype=torch.float32, device=dev)
    fl = torch.tensor([[int(flip[0]), int(flip[1])]], dtype=torch.uint8, device=dev)
    out, _, _ = augment_points(points, off, off, n, xf, flip=fl)
    points.copy_(out)
    return points


# ---- public mirrors of sampler/preprocess.py -------------------------------------------------------------------------------
def _flip_boxes_y(gt_boxes):                                               # :835-839
    gt_boxes[:, 1] = -gt_boxes[:, 1]
    gt_boxes[:, -1] = -gt_boxes[:, -1] + np.pi
    if gt_boxes.shape[1] > 7:
        gt_boxes[:, 7] = -gt_boxes[:, 7]


def _flip_boxes_x(gt_boxes):                                               # :846-852
    gt_boxes[:, 0] = -gt_boxes[:, 0]
    gt_boxes[:, -1] = -gt_boxes[:, -1] + 2 * np.pi
    if gt_boxes.shape[1] > 7:
        gt_boxes[:, 6] = -gt_boxes[:, 6]


def _draw_flip(probability):
    return bool(np.random.choice([False, True], replace=False, p=[1 - probability, probability]))


def random_flip(gt_boxes, points, probability=0.5):
    """sampler/preprocess.py:816-826."""
    enable = _draw_flip(probability)
    if enable:
        _flip_boxes_y(gt_boxes)
        _one_frame_pass(points, flip=(True, False))
    return gt_boxes, points


def random_flip_both(gt_boxes, points, probability=0.5):
    """sampler/preprocess.py:829-854."""
    fy = _draw_flip(probability)
    if fy:
        _flip_boxes_y(gt_boxes)
    fx = _draw_flip(probability)
    if fx:
        _flip_boxes_x(gt_boxes)
    if fy or fx:
        _one_frame_pass(points, flip=(fy, fx))
    return gt_boxes, points


def _rotate_boxes(gt_boxes, noise_rotation):                               # :803-812
    gt_boxes[:, :3] = rotation_points_single_angle(gt_boxes[:, :3], noise_rotation)
    if gt_boxes.shape[1] > 7:
        gt_boxes[:, 6:8] = rotation_points_single_angle(np.hstack([gt_boxes[:, 6:8], np.zeros((gt_boxes.shape[0], 1))]),
                                                        noise_rotation)[:, :2]
    gt_boxes[:, -1] += noise_rotation


def global_rotation(gt_boxes, points, rotation=np.pi / 4):
    """sampler/preprocess.py:796-813."""
    if not isinstance(rotation, list):
        rotation = [-rotation, rotation]
    noise_rotation = np.random.uniform(rotation[0], rotation[1])
    _one_frame_pass(points, cos=np.cos(noise_rotation), sin=np.sin(noise_rotation))
    _rotate_boxes(gt_boxes, noise_rotation)
    return gt_boxes, points


def global_scaling_v2(gt_boxes, points, min_scale=0.95, max_scale=1.05):
    """sampler/preprocess.py:857-861."""
    noise_scale = np.random.uniform(min_scale, max_scale)
    _one_frame_pass(points, scale=noise_scale)
    gt_boxes[:, :-1] *= noise_scale
    return gt_boxes, points


def _select_transform(transform, indices):
    result = np.zeros((transform.shape[0], *transform.shape[2:]), dtype=transform.dtype)
    for i in range(transform.shape[0]):
        if indices[i] != -1:
            result[i] = transform[i, indices[i]]
    return result


def _pair(v):
    return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [-v, v]


def _draw_noises(gt_boxes, rotation_perturb, center_noise_std, global_random_rot_range, num_try):
    """The three draws of noise_per_object_v3_ (:604-630), the unused ``global_rot_noises`` included."""
    num_boxes = gt_boxes.shape[0]
    rotation_perturb, grot = _pair(rotation_perturb), _pair(global_random_rot_range)
    if np.abs(grot[0] - grot[1]) >= 1e-3:
        raise NotImplementedError("global_rot_per_obj_range: a non-degenerate range (noise_per_box_v2_) is not built")
    if not isinstance(center_noise_std, (list, tuple, np.ndarray)):
        center_noise_std = [center_noise_std, center_noise_std, center_noise_std]
    center_noise_std = np.array(center_noise_std, dtype=gt_boxes.dtype)
    loc_noises = np.random.normal(scale=center_noise_std, size=[num_boxes, num_try, 3])
    rot_noises = np.random.uniform(rotation_perturb[0], rotation_perturb[1], size=[num_boxes, num_try])
    gt_grots = np.arctan2(gt_boxes[:, 0], gt_boxes[:, 1])
    np.random.uniform((grot[0] - gt_grots)[..., np.newaxis], (grot[1] - gt_grots)[..., np.newaxis], size=[num_boxes, num_try])
    return loc_noises, rot_noises


def _noise_inputs(gt_boxes, valid_mask, loc_noises, rot_noises):
    """Host arrays of one frame for both kernels."""
    from ..detector_ops import box_planes
    b32 = np.ascontiguousarray(gt_boxes, dtype=np.float32)
    return dict(corners=box2d_to_corner(b32[:, [0, 1, 3, 4, 6]]).astype(np.float32), centres2=b32[:, :2], centres3=b32[:, :3],
                valid=np.asarray(valid_mask, dtype=np.uint8), cos=np.cos(rot_noises).astype(np.float32),
                sin=np.sin(rot_noises).astype(np.float32), loc=np.ascontiguousarray(loc_noises, dtype=np.float64),
                planes=box_planes(np.ascontiguousarray(b32[:, :7])) if len(b32) else np.zeros((0, 6, 4), np.float32))


def _box3d_transform(gt_boxes, loc_transforms, rot_transforms, valid_mask):   # :470-476
    for i in range(gt_boxes.shape[0]):
        if valid_mask[i]:
            gt_boxes[i, :3] += loc_transforms[i]
            gt_boxes[i, 6] += rot_transforms[i]


def noise_per_object_v3_(gt_boxes, points=None, valid_mask=None, rotation_perturb=np.pi / 4, center_noise_std=1.0,
                         global_random_rot_range=np.pi / 4, num_try=5, group_ids=None, launch=None):
    """sampler/preprocess.py:587-709, in place: ``gt_boxes`` host numpy, ``points`` a float32 device tensor (or None)."""
    if group_ids is not None:
        raise NotImplementedError("group_ids: group sampling is not built")
    num_boxes = gt_boxes.shape[0]
    if valid_mask is None:
        valid_mask = np.ones((num_boxes,), dtype=np.bool_)
    loc_noises, rot_noises = _draw_noises(gt_boxes, rotation_perturb, center_noise_std, global_random_rot_range, num_try)
    dev = points.device if points is not None else torch.device("cuda")
    h = _noise_inputs(gt_boxes, valid_mask, loc_noises, rot_noises)
    d = {k: _up(v, v.dtype, dev) for k, v in h.items()}
    box_off = torch.tensor([0, num_boxes], dtype=torch.int32, device=dev)
    selected, st = noise_per_box_device(d["corners"], d["centres2"], d["valid"], d["cos"], d["sin"], d["loc"], box_off, launch)
    if points is not None and num_boxes:
        n = points.shape[0]
        off = torch.tensor([0, n], dtype=torch.int64, device=dev)
        xf = torch.tensor([[1.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
        out, _, st2 = augment_points(points, off, off, n, xf, planes=d["planes"], box_off=box_off, valid=d["valid"],
                                     centres=d["centres3"], rot_cos=d["cos"], rot_sin=d["sin"], loc=d["loc"], selected=selected,
                                     launch=launch)
        st = torch.cat([st, st2])
        points.copy_(out)
    sel = torch.cat([selected, st]).cpu().numpy()                         # the one host read
    aug_status_check(int(np.bitwise_or.reduce(sel[num_boxes:])), "noise_per_object_v3_")
    sel = sel[:num_boxes]
    _box3d_transform(gt_boxes, _select_transform(loc_noises, sel), _select_transform(rot_noises, sel), valid_mask)
    return sel


# ---- the whole train branch for a batch ------------------------------------------------------------------------------------
_REFUSED = ("random_crop", "add_rgb_to_points", "reference_detections", "remove_outside_points", "remove_environment",
            "random_select")


class TrainAugmenter:
    """What ``Preprocess.__init__`` reads of a ``train_preprocessor`` dict (pipelines/preprocess.py:30-55)."""

    def __init__(self, cfg, logger=None):
        get = cfg.get if hasattr(cfg, "get") else (lambda k, d=None: getattr(cfg, k, d))
        missing = [k for k in ("gt_rot_noise", "gt_loc_noise", "global_rot_noise", "global_scale_noise", "global_rot_per_obj_range",
                               "class_names") if get(k, None) is None]
        if missing:                                                        # the reference reads each of them unconditionally
            raise NotImplementedError(f"train Preprocess is built for a full train_preprocessor config; it lacks {missing}")
        for key in _REFUSED:
            if get(key, None) not in (None, False):
                raise NotImplementedError(f"{key}: not built in train mode")
        if get("npoints", -1) not in (-1, None):
            raise NotImplementedError("npoints: random_select / npoints is not built in train mode")
        self.shuffle_points = get("shuffle_points", False)
        self.remove_unknown = get("remove_unknown_examples", False)
        self.min_points_in_gt = get("min_points_in_gt", -1)
        self.gt_rotation_noise = get("gt_rot_noise")
        self.gt_loc_noise_std = get("gt_loc_noise")
        self.global_rotation_noise = get("global_rot_noise")
        self.global_scaling_noise = get("global_scale_noise")
        self.global_random_rot_range = get("global_rot_per_obj_range")
        grot = _pair(self.global_random_rot_range)
        if np.abs(grot[0] - grot[1]) >= 1e-3:
            raise NotImplementedError("global_rot_per_obj_range: a non-degenerate range (noise_per_box_v2_) is not built")
        self.remove_points_after_sample = get("remove_points_after_sample", False)
        self.class_names = list(get("class_names"))
        self.symmetry_intensity = get("symmetry_intensity", False)
        self.num_try = 100                                                 # pipelines/preprocess.py:191
        db = get("db_sampler", None)
        from .db_sampler import build_dbsampler
        self.db_sampler = build_dbsampler(db, logger=logger) if db else None
        self.last = None                                                   # device intermediates of the last batch (tests)


def augment_batch(frames, aug, launch=None, keep_debug=False):
    """The train branch of ``Preprocess.__call__`` (pipelines/preprocess.py:66-254) for a list of frames.

    ``frames[i]`` = dict(points = [n, F] f32 device tensor, boxes = [N, D] float32 numpy, names = [N] str array,
    difficulty (optional), image_prefix, num_point_features, flip_both (NuScenesDataset: True), calib (optional)).
    Returns one dict per frame: ``points`` (device, a view of the batch's output), ``gt_boxes``, ``gt_names``,
    ``gt_classes``.  ``aug.last`` keeps ``selected``, ``owner``, ``drop_mask``, ``kept``, ``rows`` and the offsets when
    ``keep_debug``."""
    from ..detector_ops import box_planes
    B = len(frames)
    dev = frames[0]["points"].device
    F = frames[0]["points"].shape[1]
    T = aug.num_try
    work = []
    # ---- round 1: filters, sampling, the per-object draws (host)
    if aug.min_points_in_gt > 0:
        counts = _count_points_in_gt(frames, dev)
    for f, fr in enumerate(frames):
        boxes, names = np.asarray(fr["boxes"]), np.array(fr["names"]).reshape(-1)
        difficulty = np.asarray(fr["difficulty"]) if fr.get("difficulty") is not None else np.zeros([boxes.shape[0]], np.int32)
        sel = np.array([i for i, x in enumerate(names) if x not in ["DontCare", "ignore"]], dtype=np.int64)
        keep = np.zeros(len(names), dtype=bool)
        keep[sel] = True
        if aug.remove_unknown:
            keep &= difficulty != -1
        if aug.min_points_in_gt > 0:
            keep &= counts[f] >= aug.min_points_in_gt
        boxes, names = boxes[keep], names[keep]
        mask = np.array([n in aug.class_names for n in names], dtype=np.bool_)
        sampled_points, drop_boxes = None, None
        if aug.db_sampler:
            sd = aug.db_sampler.sample_all(fr.get("image_prefix"), boxes, names, fr.get("num_point_features", F), False,
                                           gt_group_ids=None, calib=fr.get("calib"))
            if sd is not None:
                names = np.concatenate([names, sd["gt_names"]], axis=0)
                boxes = np.concatenate([boxes, sd["gt_boxes"]])
                mask = np.concatenate([mask, sd["gt_masks"]], axis=0)
                sampled_points = np.ascontiguousarray(sd["points"], dtype=np.float32)
                if aug.remove_points_after_sample:
                    drop_boxes = np.ascontiguousarray(sd["gt_boxes"], dtype=np.float32)
        boxes = np.array(boxes, copy=True)
        loc_noises, rot_noises = _draw_noises(boxes, aug.gt_rotation_noise, aug.gt_loc_noise_std, aug.global_random_rot_range, T)
        work.append(dict(boxes=boxes, names=names, mask=mask, sampled_points=sampled_points, drop_boxes=drop_boxes,
                         loc=loc_noises, rot=rot_noises, h=_noise_inputs(boxes, mask, loc_noises, rot_noises)))
    # ---- the batch's device arrays
    clouds, ns, n_in = [], [], []
    all_sampled = [w["sampled_points"] for w in work if w["sampled_points"] is not None]
    sampled_dev = _up(np.concatenate(all_sampled, axis=0), np.float32, dev) if all_sampled else None
    s0 = 0
    for fr, w in zip(frames, work):
        k = 0 if w["sampled_points"] is None else len(w["sampled_points"])
        if k:
            clouds.append(sampled_dev[s0:s0 + k])
            s0 += k
        clouds.append(fr["points"])
        ns.append(k)
        n_in.append(k + fr["points"].shape[0])
    points = torch.cat(clouds, dim=0).contiguous()
    cat = {k: np.concatenate([w["h"][k] for w in work], axis=0) for k in work[0]["h"]}
    d = {k: _up(v, v.dtype, dev) for k, v in cat.items()}
    d["cos"], d["sin"], d["loc"] = d["cos"].reshape(-1, T), d["sin"].reshape(-1, T), d["loc"].reshape(-1, T, 3)
    nb = [len(w["boxes"]) for w in work]
    box_off = _up(np.cumsum([0] + nb), np.int32, dev)
    point_off_h = np.cumsum([0] + n_in).astype(np.int64)
    point_off = _up(point_off_h, np.int64, dev)
    R = int(sum(nb))
    reads = []
    selected, st_noise = noise_per_box_device(d["corners"], d["centres2"], d["valid"], d["cos"], d["sin"], d["loc"], box_off, launch)
    reads += [selected, st_noise]
    drop_mask = ws = kept = None
    if any(w["drop_boxes"] is not None for w in work):
        dplanes = [box_planes(w["drop_boxes"]) if w["drop_boxes"] is not None else np.zeros((0, 6, 4), np.float32) for w in work]
        drop_off = _up(np.cumsum([0] + [len(p) for p in dplanes]), np.int32, dev)
        drop_mask, kept, ws, st_count = augment_points_count(points, point_off, _up(np.array(ns), np.int64, dev),
                                                             _up(np.concatenate(dplanes), np.float32, dev), drop_off, launch)
        reads += [kept, st_count]
    host = torch.cat(reads).cpu().numpy()                                  # the one host read of the batch
    sel_h = host[:R]
    aug_status_check(host[R], "al3d_noise_per_box_f32")
    n_out = list(n_in)
    if kept is not None:
        n_out = [int(v) for v in host[R + 1:R + 1 + B]]
        aug_status_check(host[R + 1 + B], "al3d_augment_points_count_f32")
    # ---- round 2: the boxes, the global draws, the shuffle (host)
    results, flips, xf, rows, stages = [], [], [], [], []
    r0 = 0
    for f, (fr, w) in enumerate(zip(frames, work)):
        boxes, mask = w["boxes"], w["mask"]
        sel = sel_h[r0:r0 + len(boxes)]
        r0 += len(boxes)
        _box3d_transform(boxes, _select_transform(w["loc"], sel), _select_transform(w["rot"], sel), mask)
        stage = dict(noise=boxes.copy()) if keep_debug else None
        boxes, names = boxes[mask], w["names"][mask]
        gt_classes = np.array([aug.class_names.index(n) + 1 for n in names], dtype=np.int32)
        fy = _draw_flip(0.5)
        if fy:
            _flip_boxes_y(boxes)
        fx = False
        if fr.get("flip_both", True):
            fx = _draw_flip(0.5)
            if fx:
                _flip_boxes_x(boxes)
        if keep_debug:
            stage["flip"] = boxes.copy()
        rotation = aug.global_rotation_noise if isinstance(aug.global_rotation_noise, list) else _pair(aug.global_rotation_noise)
        noise_rotation = np.random.uniform(rotation[0], rotation[1])
        _rotate_boxes(boxes, noise_rotation)
        if keep_debug:
            stage["rot"] = boxes.copy()
        noise_scale = np.random.uniform(*aug.global_scaling_noise)
        boxes[:, :-1] *= noise_scale
        stages.append(stage)
        if aug.shuffle_points:
            idx = np.arange(n_out[f])
            np.random.shuffle(idx)                                         # new[k] = old[idx[k]]
            inv = np.empty(n_out[f], dtype=np.int32)
            inv[idx] = np.arange(n_out[f], dtype=np.int32)
            rows.append(inv)
        flips.append([fy, fx])
        xf.append([np.float32(np.cos(noise_rotation)), np.float32(np.sin(noise_rotation)), np.float32(noise_scale)])
        results.append(dict(gt_boxes=boxes, gt_names=names, gt_classes=gt_classes))
    out_off_h = np.cumsum([0] + n_out).astype(np.int64)
    total = int(out_off_h[-1])
    rows_dev = _up(np.concatenate(rows) if rows else np.zeros(0, np.int32), np.int32, dev) if aug.shuffle_points else None
    out, owner, st = augment_points(points, point_off, _up(out_off_h, np.int64, dev), total, _up(np.array(xf), np.float32, dev),
                                    drop_mask=drop_mask, workspace=ws, planes=d["planes"], box_off=box_off, valid=d["valid"],
                                    centres=d["centres3"], rot_cos=d["cos"], rot_sin=d["sin"], loc=d["loc"], selected=selected,
                                    flip=_up(np.array(flips), np.uint8, dev), symmetry=aug.symmetry_intensity, rows=rows_dev,
                                    want_owner=keep_debug, launch=launch)
    for f, res in enumerate(results):
        res["points"] = out[int(out_off_h[f]):int(out_off_h[f + 1])]
    aug.batch_points, aug.batch_offsets = out, out_off_h                 # the whole batch, for a loader that voxelizes it at once
    aug.last = None
    if keep_debug:
        aug_status_check(st.item(), "al3d_augment_points_f32")
        aug.last = dict(selected=sel_h, owner=owner, drop_mask=drop_mask, kept=n_out, rows=rows, point_off=point_off_h,
                        box_off=np.cumsum([0] + nb), sampled=ns, status=st, input=points, stages=stages,
                        sample_dicts=[w["sampled_points"] is not None for w in work])
    return results


def _count_points_in_gt(frames, dev):
    """``points_count_rbbox`` of every frame's boxes (box_np_ops.py:14-19) in one launch and one host read."""
    from ..selector_ops import points_in_boxes_count, pib_status_check
    from ..detector_ops import box_planes
    planes = np.concatenate([box_planes(np.ascontiguousarray(fr["boxes"], dtype=np.float32)) if len(fr["boxes"])
                             else np.zeros((0, 6, 4), np.float32) for fr in frames])
    nb = [len(fr["boxes"]) for fr in frames]
    pts = torch.cat([fr["points"] for fr in frames], dim=0).contiguous()
    poff = _up(np.cumsum([0] + [fr["points"].shape[0] for fr in frames]), np.int64, dev)
    counts, _, st = points_in_boxes_count(pts, poff, _up(planes, np.float32, dev), _up(np.cumsum([0] + nb), np.int32, dev))
    host = torch.cat([counts, st]).cpu().numpy()
    pib_status_check(host[-1])
    return np.split(host[:-1], np.cumsum(nb)[:-1])
