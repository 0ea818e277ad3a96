"""float64 restatement of det3d's learned VFE readers (numpy only).

Follows VoxelFeatureExtractor / VoxelFeatureExtractorV2 + VFELayer (det3d/models/readers/voxel_encoder.py:13-176) slot by
slot with every T slot kept (no representative row): decoration [f, xyz - mean, (|xyz|)] of ALL slots -- a padded slot is
[0..0, -mean, (0)], the reference masks only after the first layer --, linear -> folded eval BN -> ReLU, max over all T
slots, concatenation with the max, mask; the same again for a second VFE layer; the final linear -> BN -> ReLU, mask, max
over T.  num_points is clipped to [0, T] and the mean divides by max(n, 1) (the reference gives NaN for n = 0; the build
computes such a row as if every slot were padded).

``vfe_net`` also returns ``absum``: per output, the abs chain through decoration (|x| + |mean| for the subtraction) and
all layers (sum |a||w| * |s| + |b|), taken as the maximum over the T slots at every max so it dominates whichever slot
wins -- the normaliser of the GPU tests' error e = |got - ref| / absum.

``pad_in_max1=False`` restates the WRONG reading -- padded slots masked in front of vfe1, so only real slots enter its max
-- for the tests that must tell the two apart.  ``pad_in_max2=False`` is the other wrong reading: the padded slots, which
hold relu(b2) in a second VFE layer, left out of that layer's max.

``nan_rule=True`` restates what the kernel documents for NaN input (csrc/vfe.hip): ReLU is fmax(pre, 0), so a NaN
pre-activation gives 0.  A NaN in a feature past xyz therefore zeroes its own slot's vfe1 row; a NaN in x, y or z makes the
mean NaN, which zeroes every real slot's vfe1 row and the padded slots' alike, so the voxel goes on as if vfe1 had given 0
everywhere.  The reference (torch.relu, torch.max) gives NaN for such a voxel.  The abs chain drops the NaN terms with the
values.

``vfe_net_f32`` evaluates the same formula with every operation rounded to float32 (numpy float32 arrays, no fused
multiply-add) in three accumulation orders; ``e32`` is the largest of their errors against ``vfe_net`` under the same
``absum``: what a float32 evaluation of this formula costs on the case at hand, the yardstick of the GPU tests' tight gate
e <= 3 e32 + 1e-8.  Neither calls the library.
"""
import numpy as np

ORDERS = ("ascending", "descending", "matmul")


def fold_bn(gamma, beta, mean, var, eps):
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return scale, np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * scale


def fold_layers(params, prefixes, eps=1e-3):
    """state-dict style ``params`` (name -> array) -> [(W, scale, shift)] for the modules named by ``prefixes``: pairs
    (linear prefix, norm prefix).  No running statistics under the norm prefix: scale 1, shift = linear bias."""
    out = []
    for lin, norm in prefixes:
        w = np.asarray(params[lin + ".weight"], np.float64)
        if norm + ".running_var" in params:
            s, b = fold_bn(params[norm + ".weight"], params[norm + ".bias"], params[norm + ".running_mean"],
                           params[norm + ".running_var"], eps)
        else:
            s, b = np.ones(w.shape[0]), np.asarray(params[lin + ".bias"], np.float64)
        out.append((w, s, b))
    return out


def vfe_net(voxels, num_points, layers, with_distance, pad_in_max1=True, pad_in_max2=True, nan_rule=False):
    """layers: [(W [units, in], scale [units], shift [units]), ...]: the one or two VFE layers, then the final linear.
    Returns (out [M, C], absum [M, C])."""
    with np.errstate(invalid="ignore"):
        return _vfe_net(voxels, num_points, layers, with_distance, pad_in_max1, pad_in_max2, nan_rule)


def _vfe_net(voxels, num_points, layers, with_distance, pad_in_max1, pad_in_max2, nan_rule):
    v = np.asarray(voxels, np.float64)
    M, T, F = v.shape
    n = np.clip(np.asarray(num_points, np.int64), 0, T)
    real = np.arange(T)[None, :] < n[:, None]                     # [M, T]
    mask = real.astype(np.float64)[..., None]
    v = v * mask
    mean = v[:, :, :3].sum(1, keepdims=True) / np.maximum(n, 1).astype(np.float64)[:, None, None]
    parts, aparts = [v, v[:, :, :3] - mean], [np.abs(v), np.abs(v[:, :, :3]) + np.abs(mean)]
    if with_distance:
        d = np.sqrt((v[:, :, :3] ** 2).sum(-1, keepdims=True))
        parts.append(d)
        aparts.append(d)
    x, ax = np.concatenate(parts, -1), np.concatenate(aparts, -1)
    for li, (w, scale, shift) in enumerate(layers):
        w = np.asarray(w, np.float64)
        pre = np.einsum("mtk,uk->mtu", x, w) * scale + shift
        ay = np.einsum("mtk,uk->mtu", ax, np.abs(w)) * np.abs(scale) + np.abs(shift)
        if nan_rule:
            y, ay = np.fmax(pre, 0.0), np.where(np.isnan(ay), 0.0, ay)
        else:
            y = np.maximum(pre, 0.0)
        if li == len(layers) - 1:
            return (y * mask).max(1), ay.max(1)
        if (li == 0 and not pad_in_max1) or (li == 1 and not pad_in_max2):
            ymax = np.where(real[..., None], y, 0.0).max(1)
        else:
            ymax = y.max(1)
        amax = ay.max(1)
        x = np.concatenate([y, np.repeat(ymax[:, None, :], T, 1)], -1) * mask
        ax = np.concatenate([ay, np.repeat(amax[:, None, :], T, 1)], -1) * mask
    raise ValueError("no layers")


def _dot32(x, w, order):
    """[M, T, K] x [U, K] -> [M, T, U] in float32: every product rounded, then added to the rounded running sum."""
    if order == "matmul":
        return np.matmul(x, np.ascontiguousarray(w.T))
    K = x.shape[-1]
    acc = np.zeros(x.shape[:2] + (w.shape[0],), np.float32)
    for k in (range(K) if order == "ascending" else range(K - 1, -1, -1)):
        acc = acc + x[:, :, k, None] * w[None, None, :, k]
    return acc


def vfe_net_f32(voxels, num_points, layers, with_distance, order="ascending"):
    """``vfe_net``'s formula (the right reading, finite input) with every operation rounded to float32: the folded scale
    and shift rounded once, the mean summed in ascending slot order and divided by float32(max(n, 1)), every dot a
    separate multiply and add per term in ``order`` -- "ascending" k, "descending" k, or "matmul" (numpy's float32
    matmul, whatever order it takes) --, then * scale, + shift, ReLU, max.  Returns out [M, C] float32."""
    assert order in ORDERS, order
    f32 = np.float32
    v = np.asarray(voxels, f32)
    M, T, F = v.shape
    n = np.clip(np.asarray(num_points, np.int64), 0, T)
    real = np.arange(T)[None, :] < n[:, None]
    mask = real.astype(f32)[..., None]
    v = v * mask
    total = np.zeros((M, 3), f32)
    for p in range(T):
        total = total + v[:, p, :3]
    mean = (total / np.maximum(n, 1).astype(f32)[:, None])[:, None, :]
    parts = [v, v[:, :, :3] - mean]
    if with_distance:
        sq = v[:, :, :3] * v[:, :, :3]
        parts.append(np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])[..., None])
    x = np.concatenate(parts, -1)
    assert x.dtype == f32
    for li, (w, scale, shift) in enumerate(layers):
        w, scale, shift = (np.asarray(a, np.float64).astype(f32) for a in (w, scale, shift))
        y = np.maximum(_dot32(x, w, order) * scale + shift, f32(0))
        assert y.dtype == f32
        if li == len(layers) - 1:
            return (y * mask).max(1)
        x = np.concatenate([y, np.repeat(y.max(1)[:, None, :], T, 1)], -1) * mask
    raise ValueError("no layers")


def err(got, ref, absum):
    """e = max |got - ref| / absum over the outputs (0 for no rows)."""
    return float((np.abs(np.asarray(got, np.float64) - ref) / absum).max()) if ref.size else 0.0


def e32(voxels, num_points, layers, with_distance, ref=None, absum=None):
    """The largest error of the three float32 evaluations against the float64 reference, relative to ``absum``."""
    if ref is None:
        ref, absum = vfe_net(voxels, num_points, layers, with_distance)
    return max(err(vfe_net_f32(voxels, num_points, layers, with_distance, o), ref, absum) for o in ORDERS)


def gate(e_32):
    """The tight gate of the GPU tests: 3 e32 + 1e-8 (the split rule of tests/test_spconv_fp64_gpu.py)."""
    return 3.0 * e_32 + 1e-8


def bound(T, widths):
    """First-order worst case of the f32 chains relative to absum: every dot of length K rounds at most K times plus the
    fold FMA, the mean at most T + 1 times, the subtraction once; 1.25 covers the second-order terms."""
    return 1.25 * (T + sum(widths) + 5) * 2.0 ** -24


def make_case(rng, M, T, F=5, counts=None, scale=1.0, centre=(-40.0, 30.0, -2.0)):
    """Random voxels in the voxelizer's format: voxels [M,T,F] f32 zero past num_points, num_points [M] i32.  Points lie
    in a 0.1 m cell near ``centre`` (a mean far from zero), times ``scale``.  counts: explicit per-voxel counts, returned
    as given (a count above T exercises the clip; the slots then hold T points)."""
    n = rng.integers(1, T + 1, size=M) if counts is None else np.asarray(counts)
    vox = np.zeros((M, T, F), np.float32)
    for i in range(M):
        k = max(0, min(int(n[i]), T))
        pts = rng.uniform(0, 1, size=(k, F))
        pts[:, :3] = np.asarray(centre) + rng.uniform(-8, 8, 3) + rng.uniform(0, 0.1, (k, 3))
        vox[i, :k] = (pts * scale).astype(np.float32)
    return vox, np.asarray(n).astype(np.int32)


def make_layers(rng, fin, filters, use_norm=True, eps=1e-3):
    """Seeded parameters with non-trivial BN statistics, state-dict style, for VFE layers of ``filters`` (each gives
    filters[i] // 2 units) and the final linear: returns (params name -> f32 array, prefixes for ``fold_layers``) under
    VoxelFeatureExtractorV2's names (vfe_layers.<i>, linear, norm)."""
    params, prefixes, cin = {}, [], fin
    specs = [(f"vfe_layers.{i}.linear", f"vfe_layers.{i}.norm", f // 2) for i, f in enumerate(filters)]
    specs.append(("linear", "norm", filters[-1]))
    for lin, norm, units in specs:
        params[lin + ".weight"] = (rng.normal(0, 1, size=(units, cin)) / np.sqrt(cin)).astype(np.float32)
        if use_norm:
            params[norm + ".weight"] = rng.uniform(0.5, 1.5, units).astype(np.float32)
            params[norm + ".bias"] = rng.normal(0, 0.5, units).astype(np.float32)
            params[norm + ".running_mean"] = rng.normal(0, 0.3, units).astype(np.float32)
            params[norm + ".running_var"] = rng.uniform(0.5, 2.0, units).astype(np.float32)
        else:
            params[lin + ".bias"] = rng.normal(0, 0.5, units).astype(np.float32)
        prefixes.append((lin, norm))
        cin = 2 * units if lin != "linear" else units
    return params, prefixes
