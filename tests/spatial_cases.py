"""The inputs shared by tests/test_spatial_cases_cpu.py (C oracle against numpy brute force and
scipy's Dijkstra) and tests/test_spatial_edges_gpu.py (the kNN / adjacency / shortest-path kernels
of csrc/apsp_kernels.hip against the oracle).

Only inputs are built here.  ``point_case(label)`` returns ``(label, xy, kq, rows)`` for a family
that goes through ``knn_2d`` first; ``table_case(label)`` returns ``(label, (knn_d, knn_i), kq,
rows)`` for a hand-made neighbour table that feeds ``apsp_knn`` directly.  ``rows`` are the source
rows to compare: every row at n <= 3000, a handful above.  Both are cached: read the arrays only.
"""
import functools

import numpy as np

ALL_ROWS_MAX_N = 3000


# ---------------------------------------------------------------- the two label paths
LDS_CAP = 158 * 1024


def sssp_lds_bytes(n):
    """Dynamic LDS of the sweep with its labels in LDS, as al3d_apsp_knn_rows_f64 sizes it:
    n 64-bit labels, then two bit sets of ceil(n / 32) words and the 16-bit node list, the
    latter two rounded up to 16 bytes together.  The labels stay in LDS while this is <= LDS_CAP."""
    words = (n + 31) // 32
    flags = (words * 8 + n * 2 + 15) // 16 * 16
    return n * 8 + flags


def last_lds_n():
    """The largest n whose labels still live in LDS; n + 1 is the first global-label size."""
    n = LDS_CAP // 11                                 # more than 10.25 bytes a node: a lower bound
    while sssp_lds_bytes(n + 1) <= LDS_CAP:
        n += 1
    return n


MAX_N = 65535                                         # node ids are 16 bit; 65536 is refused


def _rows(n, some):
    return np.arange(n) if n <= ALL_ROWS_MAX_N else np.asarray(sorted(set(some)), dtype=np.int64)


# ---------------------------------------------------------------- point families
def _lattice(h, w):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([xx.ravel() * 0.5, yy.ravel() * 0.5], axis=1).astype(np.float64)


def _uniform(n, seed, scale=500.0):
    return np.random.default_rng(seed).uniform(0, scale, size=(n, 2))


def _stopped():
    """200 poses, each held for 1..13 frames: a run longer than kq has only zero-length neighbours."""
    rng = np.random.default_rng(13)
    poses = rng.uniform(0, 500, size=(200, 2))
    reps = rng.integers(1, 14, size=200)
    return np.repeat(poses, reps, axis=0)


STOPPED_KQ = 9


def stopped_longest_run():
    xy = _stopped()
    start = np.r_[True, np.any(xy[1:] != xy[:-1], axis=1)]
    return int(np.diff(np.r_[np.nonzero(start)[0], len(xy)]).max())


def _clusters(n):
    rng = np.random.default_rng(n)
    centres = rng.uniform(0, 5000, size=(40, 2))
    return centres[rng.integers(0, 40, size=n)] + rng.normal(size=(n, 2))


def _nonfinite(nan_at, inf_at):
    xy = _uniform(300, 300)
    xy[nan_at, 0] = np.nan
    xy[inf_at, 1] = np.inf
    return xy


OFFSET = np.array([4.0e6, 6.0e5])

_POINTS = {
    # ties at every rank: the lower index wins among kept neighbours and at the kq-th place
    "lattice-40x50-kq9": lambda: (_lattice(40, 50), 9),
    "lattice-17x31-kq5": lambda: (_lattice(17, 31), 5),
    "lattice-16x16-kq32": lambda: (_lattice(16, 16), 32),
    "stopped": lambda: (_stopped(), STOPPED_KQ),
    # large common offset: the differences cancel, dx*dx + dy*dy rounds twice
    "offset-lattice": lambda: (_lattice(17, 31) + OFFSET, 5),
    "offset-random": lambda: (_uniform(1000, 77) + OFFSET, 9),
    # components: about 97 % of the map is inf
    "clusters": lambda: (_clusters(20000), 9),
    "clusters_lds": lambda: (_clusters(3000), 9),
    # a NaN and a +inf pose, behind and inside the first kq candidates of every query
    "nonfinite": lambda: (_nonfinite(100, 200), 9),
    "nonfinite-early": lambda: (_nonfinite(3, 6), 9),
    "tiles-n5-kq32": lambda: (_uniform(5, 5), 32),   # n < kq: padded with (inf, n)
    # one uniform pool on the LDS path for the row-block test
    "uniform-n700": lambda: (_uniform(700, 700, 300.0), 9),
}
for _n in (255, 256, 512, 513):                       # the 256-thread tile edges
    for _kq in (1, 2, 32):
        _POINTS[f"tiles-n{_n}-kq{_kq}"] = (lambda n=_n, kq=_kq: (_uniform(n, 1000 * kq + n), kq))

POINT_LABELS = tuple(_POINTS)
NONFINITE_LABELS = tuple(l for l in POINT_LABELS if l.startswith("nonfinite"))
FINITE_POINT_LABELS = tuple(l for l in POINT_LABELS if l not in NONFINITE_LABELS)
CLUSTER_ROWS = (0, 7777)


@functools.lru_cache(maxsize=None)
def point_case(label):
    xy, kq = _POINTS[label]()
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    n = xy.shape[0]
    return label, xy, kq, _rows(n, CLUSTER_ROWS + (n - 1,))


# ---------------------------------------------------------------- hand-made neighbour tables
def _table(n, nbr, weight):
    """kq = 2 table: column 0 is the node itself at distance 0, column 1 the one listed neighbour
    ``nbr[a]`` (or the padding (inf, n) where ``nbr[a] < 0``) at ``weight(min, max)``."""
    a = np.arange(n, dtype=np.int64)
    nbr = np.asarray(nbr, dtype=np.int64)
    has = nbr >= 0
    d = np.zeros((n, 2), dtype=np.float64)
    i = np.stack([a, np.where(has, nbr, n)], axis=1)
    lo, hi = np.minimum(a, nbr), np.maximum(a, nbr)
    d[:, 1] = np.where(has, weight(lo, hi), np.inf)
    return d, np.ascontiguousarray(i)


def _chain(n):
    """Node a lists a - 1: one path, n - 1 rounds from either end, one frontier node per round."""
    return _table(n, np.arange(n) - 1, lambda lo, hi: 1.0 + hi * 1e-4)


def chain_weights(n):
    return 1.0 + np.arange(1, n) * 1e-4


def _star(n):
    """Every node lists node 0: degree n - 1 at the hub, a frontier of n - 1 nodes after it."""
    nbr = np.zeros(n, dtype=np.int64)
    nbr[0] = -1
    return _table(n, nbr, lambda lo, hi: 1.0 + (hi % 1000) / 7.0)


HUBS, LEAVES = 64, 250


def _chain_of_stars():
    """Hub j (node 251 j) lists hub j - 1; its 250 leaves (the next 250 nodes) list it."""
    per = LEAVES + 1
    n = HUBS * per
    a = np.arange(n)
    hub = a // per * per
    nbr = np.where(a == hub, hub - per, hub)
    return _table(n, nbr, lambda lo, hi: np.where(hi % per == 0, 1.0 + lo * 1e-3 / per,
                                                  0.5 + (hi % per) / 9.0))


_LAST_LDS = last_lds_n()

_TABLES = {
    f"chain-n{_LAST_LDS}": lambda: _chain(_LAST_LDS),              # last LDS size, exactly at the cap
    f"chain-n{_LAST_LDS + 1}": lambda: _chain(_LAST_LDS + 1),      # first global-label size
    f"chain-n{MAX_N}": lambda: _chain(MAX_N),                      # node ids beyond 15 bits
    "star-n3000": lambda: _star(3000),
    f"star-n{MAX_N}": lambda: _star(MAX_N),
    "chain_of_stars": _chain_of_stars,                             # hubs and depth, global labels
}
TABLE_LABELS = tuple(_TABLES)
CHAIN_LABELS = tuple(l for l in TABLE_LABELS if l.startswith("chain-"))
STAR_LABELS = tuple(l for l in TABLE_LABELS if l.startswith("star-"))


@functools.lru_cache(maxsize=None)
def table_case(label):
    d, i = _TABLES[label]()
    n = d.shape[0]
    some = (0, 1, n // 3, n - 1)
    if label == "chain_of_stars":
        some += ((HUBS // 2) * (LEAVES + 1), n - 2)               # a middle hub, a leaf of the last
    return label, (d, i), 2, _rows(n, some)
