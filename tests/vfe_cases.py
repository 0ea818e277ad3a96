"""Cases for the fused VFE reader's edge suite (tests/test_vfe_edges_gpu.py), with the conditions each must meet checked
on the CPU (tests/test_vfe_cases_cpu.py): the sizes the launcher accepts, one case per LDS launch shape, every point
count, the designed fixtures that tell the padded-slot rules of vfe1 and vfe2 from their wrong readings, and the NaN
cases.  Numpy only; nothing here calls the library."""
import numpy as np

import vfe_fp64 as V

LDS_LIMIT = 160 * 1024


def launch_shape(T, F, wd, filters, vpw=0):
    """(V, wpb, bytes, K1, K1p): the voxels per wave, waves per workgroup and dynamic LDS bytes that ``vfe_launch``
    (csrc/vfe.hip) arrives at.  This restates the launcher's arithmetic ONLY to choose cases that reach each of its launch
    shapes; nothing is checked against it but the choice of cases.  ``bytes`` above LDS_LIMIT: the launcher refuses."""
    units = [f // 2 for f in filters]
    U1, U2, C = units[0], (units[1] if len(units) == 2 else 0), filters[-1]
    K1 = F + 3 + int(bool(wd))
    K1p = (K1 + 3) & ~3
    fixed = K1p * U1 + 2 * U1 + (2 * U1 * U2 if U2 else 0) + 2 * U2 + C * C + 2 * C
    per_voxel = T * K1p + 4 + T * (U1 + 4) + U1 + T * (U2 + 4) + U2

    def region(v):
        return (v * per_voxel + v + 3) & ~3

    v, wpb = (vpw if vpw else 2), 8
    while (fixed + wpb * region(v)) * 4 > LDS_LIMIT and (v > 1 or wpb > 1):
        if v > 1:
            v -= 1
        else:
            wpb >>= 1
    return v, wpb, (fixed + wpb * region(v)) * 4, K1, K1p


def case(T, F, wd, filters, M, counts=None, scale=1.0, use_norm=True, seed=0):
    """A seeded case: dict(vox, num, params, prefixes, layers, T, F, wd, filters).  ``counts`` as in ``V.make_case``; by
    default random in 1..T with 0, 1, T - 1, T, T + 1, T + 9 in front (those that fit into M)."""
    rng = np.random.default_rng([T, F, int(wd), M, seed, *filters])
    if counts is None:
        counts = rng.integers(1, T + 1, size=M)
        edge = [0, 1, T - 1, T, T + 1, T + 9]
        if M >= len(edge):
            counts[:len(edge)] = edge
    vox, num = V.make_case(rng, M, T, F, counts=counts, scale=scale)
    params, prefixes = V.make_layers(rng, F + 3 + int(wd), filters, use_norm)
    return dict(vox=vox, num=num, params=params, prefixes=prefixes, layers=V.fold_layers(params, prefixes), T=T, F=F,
                wd=bool(wd), filters=list(filters))


def widths(layers):
    return [w.shape[1] for w, _, _ in layers]


# ---------------------------------------------------------------- (a) sizes: (F, with_distance, filters), T = 10, M = 257
SIZES_T, SIZES_M = 10, 257
SIZES = [(3, 0, [32]), (3, 1, [96]), (4, 0, [64]), (4, 1, [128]), (5, 0, [32, 32]), (5, 1, [32, 128]),
         (10, 0, [64, 128]), (10, 1, [96, 96]), (3, 0, [128, 32]), (10, 1, [128, 128]), (4, 0, [96, 96]), (5, 0, [96])]
ALL_FILTERS = [[32], [64], [96], [128], [32, 32], [32, 128], [64, 128], [96, 96], [128, 32], [128, 128]]


def size_case(F, wd, filters):
    return case(SIZES_T, F, wd, filters, SIZES_M)


# ---------------------------------------------------------------- (b) every count
COUNT_RUNS = [(17, [32, 128]), (17, [64]), (64, [32, 128]), (64, [64])]


def count_case(T, filters):
    """T = 17: one voxel per n = 0..17, four times over in shuffled order (the row chunks of 8 and 4 end at nr = 4, 8, 12,
    16; vfe1 computes n + 1 rows when n < T).  T = 64: n = 0, 1, 63, 64."""
    rng = np.random.default_rng(T)
    counts = np.tile(np.arange(T + 1) if T == 17 else np.array([0, 1, 63, 64]), 4)
    rng.shuffle(counts)
    return case(T, 5, T == 64, filters, len(counts), counts=counts)


# ---------------------------------------------------------------- (c) one case per LDS launch shape
# (T, F, with_distance, filters, voxels_per_wave) -> the (V, wpb) it must reach
LDS_SHAPES = [((1, 5, 0, [32], 16), (16, 8)),
              ((10, 5, 0, [32, 128], 0), (2, 8)),
              ((10, 5, 0, [128, 128], 0), (1, 8)),
              ((20, 5, 0, [128, 128], 0), (1, 4)),
              ((64, 5, 0, [32, 128], 0), (1, 2)),
              ((64, 10, 1, [128, 128], 0), (1, 1))]
LDS_M = (1, 70)
VPW16_M = (1, 15, 16, 17, 129)
VPW16_RUNS = [(1, 5, 0, [32]), (5, 5, 0, [64]), (10, 5, 0, [64])]    # voxels_per_wave = 16 gives V = 16, 16, 8


def lds_case(T, F, wd, filters, M):
    return case(T, F, wd, filters, M, seed=3)


# ---------------------------------------------------------------- (e) the padded-slot fixtures
def vfe1_pad_fixture():
    """n = 1 of 10 around (-40, 30, -2): with vfe1's weights on xyz - mean signed (+, -, +) the padded slots' -mean gives
    every unit a large positive sum, and the raw xyz weights are scaled down so the one real point stays below it.  The
    right reading lets the padded slots win vfe1's max; ``pad_in_max1=False`` is the wrong one."""
    T, F, filters = 10, 5, [32, 128]
    rng = np.random.default_rng(77)
    vox, num = V.make_case(rng, 64, T, F, counts=np.ones(64, np.int64))
    params, prefixes = V.make_layers(rng, F + 3, filters)
    w1 = params["vfe_layers.0.linear.weight"]
    w1[:, F:F + 3] = np.abs(w1[:, F:F + 3]) * np.array([1.0, -1.0, 1.0], np.float32)
    w1[:, :3] *= 0.1
    return dict(vox=vox, num=num, params=params, prefixes=prefixes, layers=V.fold_layers(params, prefixes), T=T, F=F,
                wd=False, filters=filters)


def vfe2_pad_fixture():
    """The second VFE layer's padded slots read zeros and hold relu(b2).  Here b2 is large and positive (1..3, no norm:
    scale 1, shift = bias) and every weight of w2 is negative, so a real row -- whose inputs [h1, agg1] are >= 0 -- lies
    at or below b2 in every unit: wherever n < T the padded slots win vfe2's max.  The weights are small (x 0.03) so
    that most real rows stay above 0: their values still reach the output through the pointwise half.
    ``pad_in_max2=False`` (only real rows in the max) is the wrong reading.  Counts 1..T - 1 with a few full voxels, on
    which both readings agree."""
    T, F, filters = 10, 5, [32, 128]
    rng = np.random.default_rng(78)
    counts = rng.integers(1, T, size=64)
    counts[:4] = T
    vox, num = V.make_case(rng, 64, T, F, counts=counts)
    params, prefixes = V.make_layers(rng, F + 3, filters, use_norm=False)
    params["vfe_layers.1.linear.weight"] = -np.abs(params["vfe_layers.1.linear.weight"]) * np.float32(0.03)
    params["vfe_layers.1.linear.bias"] = rng.uniform(1.0, 3.0, filters[1] // 2).astype(np.float32)
    return dict(vox=vox, num=num, params=params, prefixes=prefixes, layers=V.fold_layers(params, prefixes), T=T, F=F,
                wd=False, filters=filters)


def hidden_rows(c, upto):
    """float64 post-ReLU rows [M, T, units] of VFE layer ``upto`` (0 or 1) of case ``c`` (right reading), and the real-slot
    mask [M, T]: what the fixtures' own conditions are stated on."""
    v = c["vox"].astype(np.float64)
    M, T, _ = v.shape
    n = np.clip(c["num"].astype(np.int64), 0, T)
    real = np.arange(T)[None, :] < n[:, None]
    mask = real[..., None].astype(np.float64)
    v = v * mask
    mean = v[:, :, :3].sum(1, keepdims=True) / np.maximum(n, 1)[:, None, None]
    parts = [v, v[:, :, :3] - mean]
    if c["wd"]:
        parts.append(np.sqrt((v[:, :, :3] ** 2).sum(-1, keepdims=True)))
    x = np.concatenate(parts, -1)
    for li in range(upto + 1):
        w, s, b = c["layers"][li]
        y = np.maximum(x @ w.T * s + b, 0.0)
        x = np.concatenate([y, np.repeat(y.max(1)[:, None, :], T, 1)], -1) * mask
    return y, real


# ---------------------------------------------------------------- (f) NaN input
NAN_FILTERS = [[32, 128], [64]]


def nan_case(filters, wd):
    """M = 48, T = 10, F = 5.  Voxels 5 (n = 4), 20 (n = 10 = T) and 33 (n = 7) get a NaN: voxel 5 in feature 3 (not a
    coordinate) of slot 2, voxel 20 in y of its last slot, voxel 33 in x of slot 0; 34 (n = 3) in feature 4 of slot 0 and
    z of slot 2 at once.  Returns (case, clean voxels, affected voxel indices)."""
    T = 10
    counts = np.random.default_rng(5).integers(1, T + 1, size=48)
    counts[[5, 20, 33, 34]] = [4, T, 7, 3]
    c = case(T, 5, wd, filters, 48, counts=counts, seed=6)
    clean = c["vox"].copy()
    for v, p, f in ((5, 2, 3), (20, T - 1, 1), (33, 0, 0), (34, 0, 4), (34, 2, 2)):
        assert p < c["num"][v]
        c["vox"][v, p, f] = np.nan
    return c, clean, [5, 20, 33, 34]
