"""A numpy restatement of the train Preprocess kernels (csrc/augment.hip), written from the reference's lines
(det3d/core/sampler/preprocess.py:238-267, 450-467, 796-861, 876-959; det3d/datasets/pipelines/preprocess.py:178-247), plus
the helpers the golden generator and the tests share: the margin rule, the derived coordinate bound, and a recorder / replayer
of ``np.random``.

Arithmetic: every product and sum is an elementwise numpy operation on float32 arrays, so each is rounded on its own (no
matmul, no fused multiply-add); the ``+ loc`` steps are float32 + float64 evaluated in double and rounded once.  With
``dtype=np.float64`` the coordinate chain runs in double on the same float32 inputs and float32 cos / sin (membership is always
decided in float32): that is the yardstick of the rotation bound.
"""
import hashlib

import numpy as np

NXT = [1, 2, 3, 0]
U = 2.0 ** -24                                   # one float32 rounding: at most U * |value|


# ---- box_collision_test (sampler/preprocess.py:876-959), one candidate against K boxes, vectorised over K -------------------
def standup(c):
    return np.concatenate([c.min(-2), c.max(-2)], axis=-1)


def collide_one_vs_all(cand, corners):
    """cand [4, 2], corners [K, 4, 2], same dtype -> [K] bool."""
    K = corners.shape[0]
    out = np.zeros(K, dtype=bool)
    if K == 0:
        return out
    bs, qs = standup(cand), standup(corners)
    iw = np.minimum(bs[2], qs[:, 2]) - np.maximum(bs[0], qs[:, 0])
    ih = np.minimum(bs[3], qs[:, 3]) - np.maximum(bs[1], qs[:, 1])
    idx = np.flatnonzero((iw > 0) & (ih > 0))
    if len(idx) == 0:
        return out
    q = corners[idx]
    A, B = cand[None, :, None, :], cand[NXT][None, :, None, :]
    C, D = q[:, None, :, :], q[:, NXT][:, None, :, :]
    acd = (D[..., 1] - A[..., 1]) * (C[..., 0] - A[..., 0]) > (C[..., 1] - A[..., 1]) * (D[..., 0] - A[..., 0])
    bcd = (D[..., 1] - B[..., 1]) * (C[..., 0] - B[..., 0]) > (C[..., 1] - B[..., 1]) * (D[..., 0] - B[..., 0])
    abc = (C[..., 1] - A[..., 1]) * (B[..., 0] - A[..., 0]) > (B[..., 1] - A[..., 1]) * (C[..., 0] - A[..., 0])
    abd = (D[..., 1] - A[..., 1]) * (B[..., 0] - A[..., 0]) > (B[..., 1] - A[..., 1]) * (D[..., 0] - A[..., 0])
    hit = ((acd != bcd) & (abc != abd)).any(axis=(1, 2))

    def holds(outer, inner):                     # outer [M, 4, 2], inner [M, 4, 2]: every inner corner strictly inside
        vec = -(outer - outer[:, NXT])
        cross = vec[:, :, None, 1] * (outer[:, :, None, 0] - inner[:, None, :, 0])
        cross = cross - vec[:, :, None, 0] * (outer[:, :, None, 1] - inner[:, None, :, 1])
        return ~(cross >= 0).any(axis=(1, 2))

    b = np.broadcast_to(cand, q.shape)
    over = holds(b, q)
    over = over | (~over & holds(q, b))
    out[idx] = hit | over
    return out


def pair_margin(b, q):
    """The smallest ``|a - b| / (|a| + |b|)`` over the comparisons box_collision_test EVALUATES for one pair, in float64 and
    in its short-circuit order (inf when every compared pair is (0, 0)-free and far apart; 0 for an exact tie)."""
    b, q = np.asarray(b, np.float64), np.asarray(q, np.float64)
    worst = [np.inf]

    def cmp(x, y):
        den = abs(x) + abs(y)
        worst[0] = min(worst[0], abs(x - y) / den if den > 0 else 0.0)

    bs, qs = standup(b), standup(q)
    x, y = min(bs[2], qs[2]), max(bs[0], qs[0])
    cmp(x, y)
    if not x - y > 0:
        return worst[0]
    x, y = min(bs[3], qs[3]), max(bs[1], qs[1])
    cmp(x, y)
    if not x - y > 0:
        return worst[0]
    hit = False
    for k in range(4):
        A, B = b[k], b[(k + 1) % 4]
        for l in range(4):
            C, D = q[l], q[(l + 1) % 4]
            t = [((D[1] - A[1]) * (C[0] - A[0]), (C[1] - A[1]) * (D[0] - A[0])),
                 ((D[1] - B[1]) * (C[0] - B[0]), (C[1] - B[1]) * (D[0] - B[0]))]
            for v in t:
                cmp(*v)
            if (t[0][0] > t[0][1]) != (t[1][0] > t[1][1]):
                t2 = [((C[1] - A[1]) * (B[0] - A[0]), (B[1] - A[1]) * (C[0] - A[0])),
                      ((D[1] - A[1]) * (B[0] - A[0]), (B[1] - A[1]) * (D[0] - A[0]))]
                for v in t2:
                    cmp(*v)
                if (t2[0][0] > t2[0][1]) != (t2[1][0] > t2[1][1]):
                    hit = True
                    break
        if hit:
            return worst[0]

    def holds(outer, inner):
        for l in range(4):
            for k in range(4):
                vec = -(outer[k] - outer[(k + 1) % 4])
                x, y = vec[1] * (outer[k, 0] - inner[l, 0]), vec[0] * (outer[k, 1] - inner[l, 1])
                cmp(x, y)
                if x - y >= 0:
                    return False
        return True

    if not holds(b, q):
        holds(q, b)
    return worst[0]


def candidate(corner, centre, c, s, loc, dtype=np.float32):
    """One try's corners [4, 2]: corner - centre, the rotation with float32 cos / sin, + (centre + loc) in double."""
    d = (corner - centre).astype(dtype)
    c, s = dtype(c), dtype(s)
    xr = d[:, 0] * c + d[:, 1] * s
    yr = d[:, 0] * (-s) + d[:, 1] * c
    rot = np.stack([xr, yr], axis=1)
    return (rot.astype(np.float64) + (centre.astype(np.float64) + np.asarray(loc[:2], np.float64))).astype(np.float32)


def noise_per_box_np(corners, centres, valid, cos, sin, loc, overwrite=True, margins=None):
    """noise_per_box (:238-267).  corners [R, 4, 2] f32, centres [R, 2] f32, cos / sin [R, T] f32, loc [R, T, 3] f64 ->
    selected [R] i32.  ``margins`` (a list) receives ``(box, try, other, margin)`` of every pair whose stand-up boxes
    are compared; ``overwrite=False`` leaves box_corners as they were (to show that the overwrite matters)."""
    cur = np.array(corners, dtype=np.float32, copy=True)
    R, T = cos.shape
    sel = -np.ones(R, dtype=np.int32)
    for i in range(R):
        if not valid[i]:
            continue
        for t in range(T):
            cand = candidate(cur[i], centres[i], cos[i, t], sin[i, t], loc[i, t])
            hits = collide_one_vs_all(cand, cur)
            hits[i] = False
            if margins is not None:
                for j in range(R):
                    if j != i:
                        margins.append((i, t, j, pair_margin(cand, cur[j])))
            if not hits.any():
                sel[i] = t
                if overwrite:
                    cur[i] = cand
                break
    return sel


# ---- membership (geometry.py:290-303): !(sign >= 0) on all six planes, float32 -------------------------------------------------
def inside_np(xyz, planes, chunk=4096):
    P, R = xyz.shape[0], planes.shape[0]
    out = np.zeros((P, R), dtype=bool)
    for a in range(0, P, chunk):
        p = xyz[a:a + chunk].astype(np.float32)
        x, y, z = p[:, None, None, 0], p[:, None, None, 1], p[:, None, None, 2]
        with np.errstate(invalid="ignore"):
            sign = ((x * planes[None, ..., 0] + y * planes[None, ..., 1]) + z * planes[None, ..., 2]) + planes[None, ..., 3]
            out[a:a + chunk] = (~(sign >= 0)).all(-1)
    return out


def sign_margin_ok(xyz, planes, tol=1e-4):
    """tools/gen_golden_gt_database.py's rule: in float64, inside pairs have sign < -tol |n| on all planes, outside pairs
    sign > tol |n| on at least one -> [P, R] bool."""
    x = xyz.astype(np.float64)
    n, d = planes[..., :3].astype(np.float64), planes[..., 3].astype(np.float64)
    s = np.einsum("pc,bkc->pbk", x, n) + d[None]
    s /= np.linalg.norm(n, axis=-1)[None]
    return (s < -tol).all(-1) | (s > tol).any(-1)


def rot3(x, y, z, c, s):
    """points @ [[c, -s, 0], [s, c, 0], [0, 0, 1]], three products and two sums per coordinate."""
    zero, one = x.dtype.type(0), x.dtype.type(1)
    return (x * c + y * s) + z * zero, (x * (-s) + y * c) + z * zero, (x * zero + y * zero) + z * one


def augment_points_np(points, n_sampled, planes, valid, centres, cos, sin, loc, selected, flip, gcos, gsin, scale, symmetry,
                      drop_planes=None, perm=None, dtype=np.float32):
    """One frame of the fused point pass -> (out [kept, F], owner [P], drop [P] bool).  ``perm``: out[k] = kept[perm[k]]."""
    points = np.asarray(points, np.float32)
    P = points.shape[0]
    drop = np.zeros(P, dtype=bool)
    if drop_planes is not None and len(drop_planes):
        drop = inside_np(points[:, :3], drop_planes).any(1)
        drop[:n_sampled] = False
    owner = -np.ones(P, dtype=np.int32)
    if len(planes):
        m = inside_np(points[:, :3], planes) & np.asarray(valid, bool)[None, :]
        owner = np.where(m.any(1), m.argmax(1), -1).astype(np.int32)
    xyz = points[:, :3].astype(dtype)
    own = np.flatnonzero(owner >= 0)
    if len(own):
        r = owner[own]
        sel = np.asarray(selected)[r]
        ok = sel >= 0
        c = np.where(ok, cos[r, np.maximum(sel, 0)], np.float32(1)).astype(dtype)
        s = np.where(ok, sin[r, np.maximum(sel, 0)], np.float32(0)).astype(dtype)
        l = np.where(ok[:, None], loc[r, np.maximum(sel, 0)], 0.0)
        ctr = centres[r].astype(dtype)
        d = xyz[own] - ctr
        xr, yr, zr = rot3(d[:, 0], d[:, 1], d[:, 2], c, s)
        q = np.stack([xr, yr, zr], axis=1) + ctr
        q = (q.astype(np.float64) + l).astype(dtype)
        xyz[own] = q
    x, y, z = xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy()
    if flip[0]:
        y = -y
    if flip[1]:
        x = -x
    x, y, z = rot3(x, y, z, dtype(np.float32(gcos)), dtype(np.float32(gsin)))
    sc = dtype(np.float32(scale))
    out = points.astype(dtype) if dtype != np.float32 else points.copy()
    out[:, 0], out[:, 1], out[:, 2] = x * sc, y * sc, z * sc
    if symmetry:
        out[:, -1] = out[:, -1] - dtype(0.5)
    out = out[~drop]
    if perm is not None:
        out = out[perm]
    return out, owner, drop


def coord_bound(points, centres, loc, scale):
    """The derived bound of tests/test_train_preprocess_gpu.py (see its docstring) for one frame, a scalar."""
    M = float(np.abs(points[:, :3]).max()) if len(points) else 0.0
    C = float(np.abs(centres).max()) if len(centres) else 0.0
    L = float(np.abs(loc).max()) if np.size(loc) else 0.0
    r2 = np.sqrt(2.0)
    D = M + C
    Mo = r2 * D + C + L
    e_obj = U * (r2 * D + 2 * D + r2 * D + (r2 * D + C) + Mo)
    e_rot = r2 * e_obj + U * (2 * Mo + r2 * Mo)
    s = abs(float(scale))
    return s * e_rot + U * s * r2 * Mo


# ---- np.random: record what the reference draws, replay it, and digest the state -------------------------------------------------
def state_digest():
    st = np.random.get_state()
    h = hashlib.sha256()
    h.update(st[1].tobytes())
    h.update(repr(st[2:]).encode())
    return h.hexdigest()


_NAMES = ("normal", "uniform", "choice", "shuffle")


class RecordRandom:
    """Wraps np.random's normal / uniform / choice / shuffle; ``self.log`` = [(name, float64 array)].  A 2-D shuffle is
    recorded as the index permutation it applied: the state is saved, an index array is shuffled, the state is put back, the
    rows are shuffled, and the two are asserted equal."""

    def __init__(self, pin_int_choice=True):
        self.log, self.pin = [], pin_int_choice

    def __enter__(self):
        self._orig = {n: getattr(np.random, n) for n in _NAMES}
        o = self._orig

        def normal(*a, **k):
            v = o["normal"](*a, **k)
            self.log.append(("normal", np.array(v, dtype=np.float64)))
            return v

        def uniform(*a, **k):
            v = o["uniform"](*a, **k)
            self.log.append(("uniform", np.array(v, dtype=np.float64)))
            return v

        def choice(a, *args, **k):
            if self.pin and np.ndim(a) == 0:                  # the loader's sweep order: list order, not a draw
                return np.arange(a)[:args[0] if args else k["size"]]
            v = o["choice"](a, *args, **k)
            self.log.append(("choice", np.array(v, dtype=np.float64)))
            return v

        def shuffle(x):
            if np.ndim(x) == 2:
                st = np.random.get_state()
                idx = np.arange(len(x))
                o["shuffle"](idx)
                np.random.set_state(st)
                before = x.copy()
                o["shuffle"](x)
                assert np.array_equal(before[idx].view(np.uint32), x.view(np.uint32)), "index shuffle != row shuffle"
                self.log.append(("shuffle", idx.astype(np.float64)))
            else:
                o["shuffle"](x)
                self.log.append(("shuffle", np.array(x, dtype=np.float64)))

        np.random.normal, np.random.uniform, np.random.choice, np.random.shuffle = normal, uniform, choice, shuffle
        return self

    def __exit__(self, *a):
        for n, f in self._orig.items():
            setattr(np.random, n, f)


class ReplayRandom:
    """Feeds a recorded log back: each call must be the recorded kind and shape, in order."""

    def __init__(self, log):
        self.log, self.pos = list(log), 0

    def _next(self, name, shape=None):
        assert self.pos < len(self.log), f"more draws than recorded ({name})"
        n, v = self.log[self.pos]
        self.pos += 1
        assert n == name, f"draw {self.pos - 1}: {name} asked, {n} recorded"
        if shape is not None:
            assert tuple(v.shape) == tuple(shape), f"draw {self.pos - 1} ({name}): shape {shape} asked, {v.shape} recorded"
        return v

    def __enter__(self):
        self._orig = {n: getattr(np.random, n) for n in _NAMES}

        def normal(loc=0.0, scale=1.0, size=None):
            return self._next("normal", () if size is None else size).copy()

        def uniform(low=0.0, high=1.0, size=None):
            v = self._next("uniform", () if size is None else size)
            return float(v) if size is None else v.copy()

        def choice(a, *args, **k):
            if np.ndim(a) == 0:
                return np.arange(a)[:args[0] if args else k["size"]]
            v = self._next("choice", ())
            return np.asarray(a)[int(v)] if not isinstance(a[0], (bool, np.bool_)) else np.bool_(v)

        def shuffle(x):
            v = self._next("shuffle", (len(x),))
            assert np.ndim(x) == 1
            x[:] = v.astype(x.dtype)

        np.random.normal, np.random.uniform, np.random.choice, np.random.shuffle = normal, uniform, choice, shuffle
        return self

    def __exit__(self, *a):
        for n, f in self._orig.items():
            setattr(np.random, n, f)
        if a[0] is None:
            assert self.pos == len(self.log), f"{len(self.log) - self.pos} recorded draws were not asked for"


def pack_log(log):
    """-> (kinds [n] str, sizes [n] i64 of the flattened values, ndims / shapes, values) arrays for an npz."""
    kinds = np.array([k for k, _ in log])
    shapes = [v.shape for _, v in log]
    nd = np.array([len(s) for s in shapes], dtype=np.int64)
    dims = np.array([d for s in shapes for d in s], dtype=np.int64)
    vals = np.concatenate([v.reshape(-1) for _, v in log]) if log else np.zeros(0)
    return kinds, nd, dims, vals


def unpack_log(kinds, nd, dims, vals):
    log, d0, v0 = [], 0, 0
    for k, n in zip(kinds, nd):
        shape = tuple(int(v) for v in dims[d0:d0 + n])
        d0 += n
        size = int(np.prod(shape)) if shape else 1
        log.append((str(k), vals[v0:v0 + size].reshape(shape)))
        v0 += size
    return log
