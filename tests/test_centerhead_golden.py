"""CPU: the float64 restatement tests/center_fp64.py against the reference coder's golden (tests/golden/centerhead.npz,
recorded by tools/gen_golden_centerhead.py from ``CenterPointBBoxCoder.decode`` and ``circle_nms``), and the reference's
float-division cell coordinates against integer ``//`` and ``%``.

Bounds (derived; u = 2^-24).  The golden is float32 torch arithmetic; the restatement is float64 on the same float32
inputs, with the recorded float32 sigmoid as its scores (so every ordering decision is made on the reference's own
numbers):
  * x, y = (cell + reg) * out_size_factor * voxel + pc: four float32 roundings of values below 16 in magnitude, plus the
    float32 representation of the voxel size (relative u) on a product below 16                 -> 5 * u * 16
  * height, vel: gathered                                                                      -> 0
  * dim = exp(.): torch's float32 exp is within 1 ulp, plus its rounding; a host exp one ulp from the golden's is handled
    by the allowance, not failed                                                                -> 2 * 2u relative
  * rot = atan2(.): within 2 ulp of a value <= pi                                               -> 2 * 2^-22
"""
import os

import numpy as np

import center_fp64 as C

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "centerhead.npz"))
U = 2.0 ** -24


def _case(name):
    ncls, K, has_vel, has_reg, thr, radius, post = G[f"{name}.cfg"]
    return int(ncls), int(K), bool(has_vel), bool(has_reg), float(thr), float(radius), int(post)


def _decode(name, i, dim):
    ncls, K, has_vel, has_reg, thr, _, _ = _case(name)
    geom = G["geom"]
    return C.decode(G[f"{name}.sigmoid"][i], G[f"{name}.reg"][i] if has_reg else None, G[f"{name}.height"][i], dim,
                    G[f"{name}.rot"][i], G[f"{name}.vel"][i] if has_vel else None, K=K, swapped=False,
                    out_size_factor=geom[0], voxel_size=geom[1:3], pc_range=geom[3:5], score_threshold=thr,
                    post_center_range=G["post_center_range"])


def test_decode_matches_reference_coder():
    for name in G["case_names"]:
        has_vel = _case(name)[2]
        for i in range(2):
            got = _decode(name, i, np.exp(G[f"{name}.dim"][i].astype(np.float64)))
            want = G[f"{name}.{i}.bboxes"].astype(np.float64)
            assert got["boxes"].shape == want.shape and want.shape[1] == (9 if has_vel else 7) and len(want) > 20
            assert np.array_equal(got["scores"], G[f"{name}.{i}.scores"].astype(np.float64)), "survivors / order"
            assert np.array_equal(got["labels"], G[f"{name}.{i}.labels"].astype(np.int64))
            err = np.abs(got["boxes"] - want)
            assert np.all(err[:, :2] <= 5 * U * 16), err[:, :2].max()
            assert np.all(err[:, 2] == 0)
            assert np.all(err[:, 3:6] <= 4 * U * want[:, 3:6]), (err[:, 3:6] / want[:, 3:6]).max()
            assert np.all(err[:, 6] <= 2 * 2.0 ** -22), err[:, 6].max()
            assert np.all(err[:, 7:] == 0)


def test_circle_nms_matches_reference():
    for name in G["case_names"]:
        _, _, _, _, _, radius, post = _case(name)
        for i in range(2):
            xy = G[f"{name}.{i}.bboxes"][:, :2].astype(np.float64)
            keep = C.circle_nms(xy, radius, post)
            assert keep == G[f"{name}.{i}.circle_keep"].tolist()


def test_axes_are_not_interchangeable():
    """The fixtures are 40 x 24: reading the map with the axes swapped must not reproduce the golden."""
    name = G["case_names"][0]
    ncls, K, has_vel, has_reg, thr, _, _ = _case(name)
    geom = G["geom"]
    got = C.decode(G[f"{name}.sigmoid"][0], G[f"{name}.reg"][0], G[f"{name}.height"][0], G[f"{name}.exp_dim"][0], G[f"{name}.rot"][0],
                   G[f"{name}.vel"][0], K=K, swapped=True, out_size_factor=geom[0], voxel_size=geom[1:3], pc_range=geom[3:5],
                   score_threshold=thr, post_center_range=G["post_center_range"])
    want = G[f"{name}.0.bboxes"]
    assert got["boxes"].shape != want.shape or np.abs(got["boxes"][:, :2] - want[:, :2]).max() > 0.1


def test_float_division_coordinates_equal_integer_division():
    """coder :87-90 takes the cell's first coordinate as ``(ind.float() / float(width)).int()``.  For every width 1..4096
    and every row 0..4095 whose last cell has an index below 2^24 (exact in float32) that equals ``ind // width`` at the
    last cell of the row (the quotient closest to the next integer from below) and at the first (an exact quotient);
    the class ``(ind / K).int()`` is the same expression."""
    rows = np.arange(4096, dtype=np.int64)
    for width in range(1, 4097):
        last = rows * width + (width - 1)
        last = last[last < (1 << 24)]
        first = last - (width - 1)
        w32 = np.float32(width)
        assert np.array_equal((last.astype(np.float32) / w32).astype(np.int32), last // width), width
        assert np.array_equal((first.astype(np.float32) / w32).astype(np.int32), first // width), width
