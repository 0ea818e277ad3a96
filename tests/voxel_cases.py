"""Named deterministic cases for the hard voxelizer (csrc/voxelize.hip), each built for one branch of its passes, and the
numpy restatements they are judged by.  tests/test_voxel_cases_cpu.py proves on the CPU that every case tells the right
voxelizer from a plausible wrong one; tests/test_voxel_edges_gpu.py runs the HIP code on them.

A structural case is a sequence of cell ids per frame (``-1``: a point outside the grid) turned into points well inside
those cells of a small 64 x 64 x 8 grid; the arithmetic cases put coordinates a few ulps round every cell edge of the real
geometries."""
import numpy as np

SMALL = dict(range=[-3.2, -3.2, -2.0, 3.2, 3.2, 2.0], vsize=[0.1, 0.1, 0.5], grid=[64, 64, 8])
# name -> (range, voxel size, grid, max_points, nfeat): the voxel_generator blocks of the configurations
GEOMETRIES = {
    "nuscenes": dict(range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], vsize=[0.1, 0.1, 0.2], grid=[1024, 1024, 40],
                     max_points=10, nfeat=5),
    "bevfusion": dict(range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], vsize=[0.075, 0.075, 0.2], grid=[1440, 1440, 40],
                      max_points=10, nfeat=5),
    "pointpillars": dict(range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], vsize=[0.2, 0.2, 8.0], grid=[512, 512, 1],
                         max_points=20, nfeat=5),
    "kitti": dict(range=[0.0, -39.68, -3.0, 69.12, 39.68, 1.0], vsize=[0.16, 0.16, 4.0], grid=[432, 496, 1],
                  max_points=32, nfeat=4),
}
ARITH_MAX_VOXELS = 30000
LENGTHS = [1, 63, 64, 65, 0, 0, 127, 300, 2]              # frame_edges
CAP = 50                                                  # cap_in_batch, stale_grid
GATHER_MAX_POINTS = [1, 3, 9, 10, 20, 32]
GATHER_NFEAT = [3, 4, 5, 6]


# ----------------------------------------------------------------------------------------------- numpy restatements
def grid_of(geom):
    r, vs = np.asarray(geom["range"], np.float32), np.asarray(geom["vsize"], np.float32)
    return np.round((r[3:] - r[:3]) / vs).astype(np.int64)


def _ftz(a):
    return np.where(np.abs(a) < np.float32(2.0 ** -126), np.float32(0) * a, a)


def axis_index(v, lo, vs, mode="f32"):
    """floor((v - lo) / vs) of float32 values on one axis, as a float array.  ``f32``: numpy float32, the statement the
    kernel must equal; the others are the wrong ways a kernel could take: ``recip`` multiplies with float32(1)/vs, ``f64``
    computes in double, ``ftz`` flushes float32 denormals to zero at every step."""
    v = np.asarray(v, np.float32)
    lo32, vs32 = np.float32(lo), np.float32(vs)
    with np.errstate(all="ignore"):
        if mode == "f32":
            return np.floor((v - lo32) / vs32)
        if mode == "recip":
            return np.floor((v - lo32) * (np.float32(1) / vs32))
        if mode == "f64":
            return np.floor((v.astype(np.float64) - np.float64(lo32)) / np.float64(vs32))
        if mode == "ftz":
            return np.floor(_ftz(_ftz(_ftz(v) - lo32) / vs32))
    raise ValueError(mode)


def cells_of(pts, geom, mode="f32"):
    """Flat cell id (z * gy + y) * gx + x per point, -1 outside the grid (NaN included)."""
    g = np.asarray(geom["grid"], np.int64)
    f = np.stack([axis_index(pts[:, d], geom["range"][d], geom["vsize"][d], mode) for d in range(3)], 1)
    with np.errstate(invalid="ignore"):
        ok = np.all((f >= 0) & (f < g[None].astype(f.dtype)), axis=1)
    i = np.where(ok[:, None], f, 0).astype(np.int64)
    return np.where(ok, (i[:, 2] * g[1] + i[:, 1]) * g[0] + i[:, 0], -1)


def cell_coords_zyx(cells, geom):
    gx, gy, _ = geom["grid"]
    cells = np.asarray(cells, np.int64).reshape(-1)
    return np.stack([cells // (gx * gy), (cells // gx) % gy, cells % gx], 1).astype(np.int32)


def first_appearance(cells):
    """Distinct cells (>= 0) in the order of their first point, with that point's index."""
    u, idx = np.unique(cells, return_index=True)
    keep = u >= 0
    order = np.argsort(idx[keep], kind="stable")
    return u[keep][order], idx[keep][order]


def model_voxelize(pts, cells, geom, max_points, max_voxels, variant="ref", arrival=None):
    """Sequential restatement of one frame -> (voxels, coords_zyx, num_points, feat) like ``oracle.voxelize``.
    variant ``ref`` is the contract; the others are wrong on purpose: ``clamp`` keeps the points of a cell beyond the cap
    (in the last kept voxel), ``break`` stops at the first cell beyond the cap, ``by_cell_id`` keeps the max_voxels lowest
    cell ids instead of the first to appear.  ``arrival``: a function on a voxel's ascending point indices; the voxel then
    keeps the first max_points of the list it returns (the bucket's arrival order) instead of index order."""
    order, vid, members = [], {}, []
    allowed = set(np.unique(cells[cells >= 0])[:max_voxels].tolist()) if variant == "by_cell_id" else None
    for i, c in enumerate(cells.tolist()):
        if c < 0:
            continue
        v = vid.get(c)
        if v is None:
            full = (c not in allowed) if allowed is not None else len(order) >= max_voxels
            if full and variant == "break":
                break
            if full and variant == "clamp" and order:
                v = len(order) - 1
            elif full:
                vid[c] = -2
                continue
            else:
                v = len(order)
                order.append(c)
                members.append([])
            vid[c] = v
        elif v == -2:
            continue
        members[v].append(i)
    m, f = len(order), pts.shape[1]
    voxels = np.zeros((m, max_points, f), np.float32)
    num = np.zeros(m, np.int32)
    for v, idx in enumerate(members):
        if arrival is not None:
            idx = arrival(idx)
        sel = idx[:max_points]
        voxels[v, :len(sel)] = pts[sel]
        num[v] = len(sel)
    s = np.zeros((m, f), np.float32)
    for t in range(max_points):                      # the slot-order float32 sum, zero slots included
        s = s + voxels[:, t, :]
    with np.errstate(all="ignore"):
        feat = s / num.astype(np.float32)[:, None]
    return voxels, cell_coords_zyx(order, geom), num, feat


def lane_skip_leaders(frame_cells, compare_frame=True):
    """The first-index pass as the kernel runs it: a lane whose (cell, frame) also sits in one of the four lanes below it in
    its 64-lane wave issues no atomicMin.  -> {(frame, cell): smallest frame-local index that was issued}.  With
    ``compare_frame=False`` the skip looks at the cell alone: the wrong kernel the frame_edges case must expose."""
    cells = np.concatenate([np.asarray(c, np.int64) for c in frame_cells]) if frame_cells else np.zeros(0, np.int64)
    frame = np.concatenate([np.full(len(c), b, np.int64) for b, c in enumerate(frame_cells)])
    start = np.concatenate([[0], np.cumsum([len(c) for c in frame_cells])])
    first = {}
    for i in range(len(cells)):
        if cells[i] < 0:
            continue
        lane = i % 64
        dup = any(lane >= k and cells[i - k] == cells[i] and (frame[i - k] == frame[i] or not compare_frame)
                  for k in range(1, 5))
        if not dup:
            key = (int(frame[i]), int(cells[i]))
            first[key] = min(first.get(key, 1 << 31), i - int(start[frame[i]]))
    return first


def true_leaders(frame_cells):
    out = {}
    for b, c in enumerate(frame_cells):
        u, idx = first_appearance(np.asarray(c, np.int64))
        out.update({(b, int(k)): int(v) for k, v in zip(u, idx)})
    return out


def stale_grid_order(x_cells, y_cells, stale_only=None):
    """Voxel order of frame Y on a first-index grid that still holds frame X's leaders: first[cell] = min(X's leader, Y's),
    a point is a leader iff first[its cell] == its own index.  ``stale_only``: the cells X left behind (default: all of X's).
    -> the cells of Y's leader points in index order (== first_appearance(y_cells)[0] on a clean grid)."""
    xu, xi = first_appearance(np.asarray(x_cells, np.int64))
    first = {int(c): int(i) for c, i in zip(xu, xi) if stale_only is None or int(c) in stale_only}
    yu, yi = first_appearance(np.asarray(y_cells, np.int64))
    for c, i in zip(yu, yi):
        first[int(c)] = min(first.get(int(c), 1 << 31), int(i))
    return [int(c) for i, c in enumerate(np.asarray(y_cells).tolist()) if c >= 0 and first[int(c)] == i]


def dropped_by_cap(cells, max_voxels):
    return set(first_appearance(np.asarray(cells, np.int64))[0][max_voxels:].tolist())


# ----------------------------------------------------------------------------------------------- points from cell ids
def points_in(rng, cell_ids, nfeat=5, geom=SMALL):
    """One point per entry: well inside that cell (0.2 .. 0.8 of the voxel on every axis), or beyond range_max for -1;
    the other features are N(0, 30): sums of them depend on the order of the addends."""
    ids = np.asarray(cell_ids, np.int64).reshape(-1)
    gx, gy, _ = geom["grid"]
    lo, hi, vs = np.array(geom["range"][:3]), np.array(geom["range"][3:]), np.array(geom["vsize"])
    safe = np.maximum(ids, 0)
    ijk = np.stack([safe % gx, (safe // gx) % gy, safe // (gx * gy)], 1).astype(np.float64)
    xyz = lo + (ijk + rng.uniform(0.2, 0.8, (len(ids), 3))) * vs
    xyz[ids < 0] = hi + 1.0 + rng.uniform(0, 5, (int((ids < 0).sum()), 3))
    return np.concatenate([xyz, rng.normal(0, 30, (len(ids), nfeat - 3))], 1).astype(np.float32)


def _case(name, frame_cells, rng, max_points, max_voxels, nfeat=5, tail_cells=None, geom=SMALL):
    frames = [points_in(rng, c, nfeat, geom) for c in frame_cells]
    return dict(name=name, geom=geom, frames=frames, cells=[np.asarray(c, np.int64) for c in frame_cells],
                max_points=max_points, max_voxels=max_voxels, nfeat=nfeat,
                tail=None if tail_cells is None else points_in(rng, tail_cells, nfeat, geom))


def _distinct(rng, n, geom=SMALL, exclude=()):
    total = int(np.prod(geom["grid"]))
    pool = np.setdiff1d(np.arange(total), np.asarray(list(exclude), np.int64))
    return rng.choice(pool, n, replace=False)


# ----------------------------------------------------------------------------------------------- (a) cap_in_batch
def cap_in_batch():
    """Five frames under max_voxels = 50 with 200, exactly 50, 0, 51 and 49 distinct cells.  In the capped frames the points
    of dropped cells come back later, lane by lane between points of kept cells; dropped cell number 50 has a run of 150
    (more than two waves); number 49 is the last kept."""
    rng = np.random.default_rng(101)
    C = _distinct(rng, 200).tolist()
    f0 = C[:60]
    for j in range(64):
        f0 += [C[j % 50], C[50 + j % 10]]
    f0 += [C[50]] * 150 + [C[49]] * 70 + [-1] * 3
    for j in range(60, 200):
        f0 += [C[j], C[j % 50]]
    f0 += [C[49], C[50], C[199], C[0]]
    D = _distinct(rng, 50)
    f1 = rng.permutation(np.repeat(D, 4)).tolist()
    f2 = [-1] * 37
    E = _distinct(rng, 51).tolist()
    f3 = E[:50] + [E[50], E[49], E[50], E[10], E[50]] + rng.permutation(np.repeat(E, 2)).tolist()
    F = _distinct(rng, 49)
    f4 = rng.permutation(np.repeat(F, 3)).tolist()
    return _case("cap_in_batch", [f0, f1, f2, f3, f4], rng, max_points=5, max_voxels=CAP)


# ----------------------------------------------------------------------------------------------- (b) gather_sweep
def gather_sweep(max_points, nfeat):
    """Cells of max_points - 1, max_points, max_points + 1 and 5 * max_points points scattered among 300 single-point
    cells (the frame spans several waves: bucket slots are handed out in arrival order, not index order); the second frame
    is another shuffle of the same multiset."""
    rng = np.random.default_rng(1000 * max_points + nfeat)
    C = _distinct(rng, 304)
    sizes = [max_points - 1, max_points, max_points + 1, 5 * max_points]
    base = np.concatenate([np.repeat(C[:4], sizes), C[4:]])
    frames = [rng.permutation(base).tolist(), rng.permutation(base).tolist()]
    case = _case(f"gather_{max_points}x{nfeat}", frames, rng, max_points=max_points, max_voxels=400, nfeat=nfeat)
    case["sizes"] = sizes
    return case


# ----------------------------------------------------------------------------------------------- (c) frame_edges
SHARED_AT = {0: [0], 1: [0, 62], 2: [1, 63], 3: [0, 64], 6: [1, 2, 126], 7: [2, 296], 8: [0, 1]}


def frame_edges():
    """One cell in every frame, placed so that two of its points in DIFFERENT frames sit 1, 2, 3 and 4 lanes apart inside
    one wave (and up to 3 apart across wave boundaries); everything else is single-point filler."""
    rng = np.random.default_rng(202)
    shared = int(_distinct(rng, 1)[0])
    frames = []
    for b, n in enumerate(LENGTHS):
        c = _distinct(rng, n, exclude=[shared])
        for p in SHARED_AT.get(b, []):
            c[p] = shared
        frames.append(c.tolist())
    case = _case("frame_edges", frames, rng, max_points=5, max_voxels=400)
    case["shared"] = shared
    return case


def empty_frame_cases():
    rng = np.random.default_rng(203)
    five = _distinct(rng, 3)[[0, 1, 0, 2, 1]].tolist()
    return [_case("empty_ends", [[], [], five, []], rng, max_points=5, max_voxels=CAP),     # off = [0, 0, 0, 5, 5]
            _case("no_points", [[], [], []], rng, max_points=5, max_voxels=CAP)]           # npts = 0, B = 3


# ----------------------------------------------------------------------------------------------- (d) stale_grid
def _rotated(cells, pad):
    """[body, pad * -1] -> [pad * -1, body]: the same points rotated, every cell's first index larger by ``pad``."""
    return cells, [-1] * pad + cells[:len(cells) - pad]


def stale_grid_pairs():
    """-> list of (name, [case X, case Y, ...]): the calls one resident Voxelizer(max_batch=8) sees in turn.  Every later
    call holds the cells of the earlier ones at larger frame-local indices, so a cell an earlier call failed to reset
    keeps a leader index that is not a point of that cell in the later call."""
    rng = np.random.default_rng(303)
    pad = 40
    out = []

    def body(n_cells, per_cell):
        return rng.permutation(np.repeat(_distinct(rng, n_cells), per_cell)).tolist()

    # X is capped: 80 and 65 cells under a cap of 50, so 30 and 15 cells are dropped (and must be reset all the same)
    x = [body(80, 3) + [-1] * pad, body(65, 2) + [-1] * pad]
    y = [_rotated(f, pad)[1] for f in x]
    out.append(("capped", [_case("stale_capped_x", x, rng, 5, CAP), _case("stale_capped_y", y, rng, 5, CAP)]))
    # X has rows past off[B]: in-range points of X's cells and of new ones, which no pass may put into the grid
    x = [body(40, 3) + [-1] * pad, body(30, 2) + [-1] * pad]
    tail = body(25, 2) + x[1][:30]
    y = [_rotated(x[0], pad)[1], [-1] * pad + x[1][:len(x[1]) - pad] + tail]
    out.append(("tail", [_case("stale_tail_x", x, rng, 5, 400, tail_cells=tail), _case("stale_tail_y", y, rng, 5, 400)]))
    # B = 3, then B = 8 on the same cells (frames 3..7 of the grid were never used), then B = 1
    x = [body(40, 3) + [-1] * pad for _ in range(3)]
    y = [[-1] * pad + x[j % 3][:len(x[j % 3]) - pad] for j in range(8)]
    z = [[-1] * (2 * pad) + x[0][:len(x[0]) - pad] + x[1][:60]]
    out.append(("batch_sizes", [_case("stale_b3", x, rng, 5, 400), _case("stale_b8", y, rng, 5, 400),
                                _case("stale_b1", z, rng, 5, 400)]))
    return out


# ----------------------------------------------------------------------------------------------- (e) cell_arithmetic
def edge_values(lo, vs, n):
    """float32(lo + k * vs) for k = 0..n, each moved by -3..+3 ulps: [n + 1, 7] float32."""
    base = (lo + np.arange(n + 1, dtype=np.float64) * vs).astype(np.float32)
    cols = {0: base}
    for sign, to in ((-1, -np.inf), (1, np.inf)):
        v = base
        for step in range(1, 4):
            v = np.nextafter(v, np.float32(to))
            cols[sign * step] = v
    return np.stack([cols[k] for k in range(-3, 4)], 1)


def cell_arithmetic(name):
    """One frame on a real geometry: one pass per axis walks that axis through every edge value while the other two
    coordinates are drawn from those of their own edge values that lie inside the grid (so the walked axis decides), then
    the special values one coordinate at a time."""
    geom = dict(GEOMETRIES[name])
    rng = np.random.default_rng(sum(map(ord, name)))
    lo, vs, grid, nfeat = geom["range"][:3], geom["vsize"], geom["grid"], geom["nfeat"]
    sets = [edge_values(lo[d], vs[d], grid[d]).reshape(-1) for d in range(3)]
    parts = []
    inner = []                                        # the edge values that lie inside the grid on their axis
    for d in range(3):
        k = axis_index(sets[d], lo[d], vs[d])
        inner.append(sets[d][(k >= 0) & (k < grid[d])])
    for d in range(3):
        n = len(sets[d])
        xyz = np.stack([sets[a] if a == d else rng.choice(inner[a], n) for a in range(3)], 1)
        parts.append(xyz)
    inside = np.array([lo[d] + vs[d] * (0.5 + grid[d] // 2) for d in range(3)], np.float32)
    specials = [np.nan, np.inf, -np.inf, 1e38, -1e38]
    if name == "kitti":
        specials_x = specials + [-0.0, 0.0, 1e-40, -1e-40]
    else:
        specials_x = specials
    sp = []
    for d in range(3):
        for v in (specials_x if d == 0 else specials):
            p = inside.copy()
            p[d] = np.float32(v)
            sp.append(p)
    parts.append(np.stack(sp))
    xyz = np.concatenate(parts).astype(np.float32)
    pts = np.concatenate([xyz, rng.normal(0, 30, (len(xyz), nfeat - 3)).astype(np.float32)], 1)
    return dict(name=f"arith_{name}", geom=geom, frames=[pts], cells=[cells_of(pts, geom)], max_points=geom["max_points"],
                max_voxels=ARITH_MAX_VOXELS, nfeat=nfeat, tail=None, sets=sets, n_special=len(sp))
