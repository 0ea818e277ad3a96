"""One deterministic batch for al3d_merge_sweeps_batch_range_f32 (csrc/sweeps.hip), called on raw arrays without any file,
and its per-frame references: ``oracle.merge_sweeps`` for rule 0 (det3d), oracle/bevfusion_loading.py's ``merge_sweeps``
for rule 1 (BEVFusion) and its ``points_range_filter`` for the range filter.

The five frames: an ordinary one; one whose files are all empty, in the middle; one whose every point is removed (sweeps
of close points only); one whose key-frame file is empty while its sweeps are not; and a last one whose files are all empty
(its first row is the end of the input).  4,712 input rows: the scan runs three workgroups."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import bevfusion_loading as BL  # noqa: E402

RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]           # every bound is a float32
MIN_DISTANCE = 1.0
SHIFT = np.array([2.0, -1.0, 0.5])                      # the boundary sweep's translation (rotation: identity)
TAG = 1000.0                                            # intensity of boundary point j is TAG + j
KEY_TS = 1_600_000_000_000_000                          # microseconds


def _rotation(rng):
    yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]) @
            np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def _cloud(rng, n, spread=20.0):
    return np.concatenate([rng.normal(0, spread, (n, 2)), rng.normal(-1.0, 1.5, (n, 1)), rng.uniform(0, 255, (n, 1)),
                           rng.integers(0, 32, (n, 1))], 1).astype(np.float32)


def _sweep(points, lag_us, R=None, t=None):
    """A sweep file; R is None: the file has no transform (the references get the identity, which changes no bit of a
    finite value that is not -0)."""
    return dict(points=points, timestamp=KEY_TS - lag_us, has_xform=R is not None,
                sensor2lidar_rotation=np.eye(3) if R is None else R,
                sensor2lidar_translation=np.zeros(3) if t is None else np.asarray(t, np.float64))


def boundary_points():
    """12 raw points of the boundary sweep (identity rotation, translation SHIFT): on each axis the transformed coordinate is
    exactly lo, one ulp above lo, exactly hi, one ulp below hi; the other two coordinates land well inside.
    -> (points [12, 5], inside [12] bool)."""
    lo, hi = np.asarray(RANGE[:3], np.float32), np.asarray(RANGE[3:], np.float32)
    pts, inside = [], []
    for d in range(3):
        for target, ok in ((lo[d], False), (np.nextafter(lo[d], np.float32(np.inf)), True), (hi[d], False),
                           (np.nextafter(hi[d], np.float32(-np.inf)), True)):
            want = np.array([10.0, 10.0, 0.0])
            want[d] = np.float64(target)
            raw = (want - SHIFT).astype(np.float32)
            assert np.array_equal((raw.astype(np.float64) + SHIFT).astype(np.float32).astype(np.float64), want)
            pts.append(np.concatenate([raw, [TAG + len(pts), 3.0]]).astype(np.float32))
            inside.append(ok)
    return np.stack(pts), np.array(inside)


def build():
    """-> list of five frames, each dict(key [p, 5] f32, sweeps [dict], ts)."""
    rng = np.random.default_rng(404)
    empty = np.zeros((0, 5), np.float32)
    key0 = _cloud(rng, 700)
    key0[123, 0] = np.nan                                 # kept without the range filter, dropped with it
    s1 = _cloud(rng, 900)
    s1[::7, :2] = rng.uniform(-0.99, 0.99, (len(s1[::7]), 2)).astype(np.float32)        # close to the sensor: removed
    s3 = np.concatenate([_cloud(rng, 60), boundary_points()[0], _cloud(rng, 40)])
    close_a = _cloud(rng, 300)
    close_a[:, :2] = rng.uniform(-0.99, 0.99, (300, 2)).astype(np.float32)
    close_b = _cloud(rng, 200)
    close_b[:, :2] = rng.uniform(-0.5, 0.5, (200, 2)).astype(np.float32)
    frames = [
        dict(key=key0, sweeps=[_sweep(s1, 50_000, _rotation(rng), rng.normal(0, 2, 3)),
                               _sweep(_cloud(rng, 500), 100_000),                       # no transform
                               _sweep(s3, 150_000, np.eye(3), SHIFT)]),
        dict(key=empty, sweeps=[_sweep(empty, 50_000, _rotation(rng), rng.normal(0, 2, 3)), _sweep(empty, 100_000)]),
        dict(key=empty, sweeps=[_sweep(close_a, 50_000, _rotation(rng), rng.normal(0, 2, 3)),
                                _sweep(close_b, 100_000, _rotation(rng), rng.normal(0, 2, 3))]),
        dict(key=empty, sweeps=[_sweep(_cloud(rng, 800), 50_000, _rotation(rng), rng.normal(0, 2, 3)),
                                _sweep(_cloud(rng, 1200, 30.0), 100_000, _rotation(rng), rng.normal(0, 2, 3))]),
        dict(key=empty, sweeps=[_sweep(empty, 50_000, _rotation(rng), rng.normal(0, 2, 3))]),
    ]
    for f in frames:
        f["ts"] = KEY_TS
    return frames


def time_lag(frame, sweep):
    return frame["ts"] / 1e6 - sweep["timestamp"] / 1e6


def kernel_arrays(frames):
    """The flat arrays of the C entry: raw rows, file offsets, per-file transform / flags / time lag, frame -> first file."""
    files, xform, has, lag, key, first = [], [], [], [], [], []
    for f in frames:
        first.append(len(files))
        files.append(f["key"])
        xform.append(np.zeros(12)); has.append(0); lag.append(0.0); key.append(1)
        for s in f["sweeps"]:
            files.append(s["points"])
            m = np.concatenate([s["sensor2lidar_rotation"], s["sensor2lidar_translation"][:, None]], 1).reshape(12)
            xform.append(m if s["has_xform"] else np.zeros(12))
            has.append(int(s["has_xform"])); lag.append(time_lag(f, s)); key.append(0)
    first.append(len(files))
    off = np.concatenate([[0], np.cumsum([len(p) for p in files])]).astype(np.int64)
    return dict(raw=np.concatenate(files).astype(np.float32), file_off=off, xform=np.asarray(xform, np.float64),
                has_xform=np.asarray(has, np.uint8), time_lag=np.asarray(lag, np.float64), is_key=np.asarray(key, np.uint8),
                frame_first_file=np.asarray(first, np.int32), nfiles=len(files), total=int(off[-1]), n_frames=len(frames))


def reference(oracle, frames, rule, filtered):
    """Per-frame merged clouds [n, 5] f32 under rule 0 or 1, with or without the range filter."""
    out = []
    for f in frames:
        if rule == 0:
            xf = [None]
            for s in f["sweeps"]:
                T = np.eye(4)
                T[:3, :3], T[:3, 3] = s["sensor2lidar_rotation"], s["sensor2lidar_translation"]
                xf.append(T if s["has_xform"] else None)
            lags = [0.0] + [time_lag(f, s) for s in f["sweeps"]]
            p = oracle.merge_sweeps([f["key"]] + [s["points"] for s in f["sweeps"]], xf, lags, MIN_DISTANCE)
        else:
            p = BL.merge_sweeps(f["key"], f["sweeps"], f["ts"], sweeps_num=len(f["sweeps"]), pad_empty_sweeps=False,
                                remove_close=True, radius=MIN_DISTANCE)
        out.append(BL.points_range_filter(p, RANGE) if filtered else p)
    return out


def rule1_by_hand(frame):
    """Rule 1 spelt out element by element (no matrix product: a BLAS kernel may fuse multiply and add): the float64
    rotation ((R0 x + R1 y) + R2 z) rounded to float32, then the float64 translation added and rounded again."""
    key = frame["key"].copy()
    key[:, 4] = 0
    out = [key]
    for s in frame["sweeps"]:
        p = s["points"]
        p = p[~((np.abs(p[:, 0]) < MIN_DISTANCE) & (np.abs(p[:, 1]) < MIN_DISTANCE))].copy()
        R, t = s["sensor2lidar_rotation"], s["sensor2lidar_translation"]
        x, y, z = (p[:, d].astype(np.float64) for d in range(3))
        for d in range(3):
            r = ((R[d, 0] * x + R[d, 1] * y) + R[d, 2] * z).astype(np.float32)
            p[:, d] = (r.astype(np.float64) + t[d]).astype(np.float32)
        p[:, 4] = np.float32(time_lag(frame, s))
        out.append(p)
    return np.concatenate(out)
