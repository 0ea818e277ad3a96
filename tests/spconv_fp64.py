"""Float64 reference of the sparse 3-D convolution and of FPNSpMiddleResNetFHD (numpy only).

Stated from the definition of the operation, independently of the library's rulebook kernels and of the C oracle:

  sites      submanifold: the input sites.  Strided: every output cell o with at least one active input i = o*s - p + d
             in its receptive field (d over the kernel offsets), found by enumerating the offsets per input.
  neighbours nbr[o, t] = row of the input at cell o*s - p + d_t (strided) or o + d_t - k//2 (submanifold), -1 where the
             cell is outside the grid or inactive; taps t in (dz, dy, dx) row-major order, the order of the weight
             [kz, ky, kx, Cin, Cout] flattened.  Looked up with searchsorted over the linearised cell keys.
  layer      out = sum_t X[nbr_t] @ W_t, then * scale + shift, + residual, ReLU (NaN-preserving, like torch.relu).
  normaliser the same layer on |X|, |W|, |scale|, |shift|, |residual| without ReLU: per output element the sum of
             |a*b| over every product and addend that forms it -- what an error bound of a fp32-class kernel scales with.
"""
import numpy as np


def out_shape(shape, k, s, p):
    return [(int(shape[d]) + 2 * int(p[d]) - int(k[d])) // int(s[d]) + 1 for d in range(3)]


def cell_key(coords, shape):
    """(b, z, y, x) int rows -> int64 linear cell index."""
    c = np.asarray(coords).astype(np.int64).reshape(-1, 4)
    D, H, W = [int(v) for v in shape]
    return ((c[:, 0] * D + c[:, 1]) * H + c[:, 2]) * W + c[:, 3]


def _offsets(k):
    return np.array([(a, b, c) for a in range(k[0]) for b in range(k[1]) for c in range(k[2])], dtype=np.int64)


def strided_sites(coords, shape, k, s, p):
    """Output cells of a strided layer, as [n_out, 4] int32 (b, z, y, x) in ascending cell order, and the output shape."""
    oshape = out_shape(shape, k, s, p)
    c = np.asarray(coords).astype(np.int64).reshape(-1, 4)
    s3, p3 = np.asarray(s, np.int64), np.asarray(p, np.int64)
    keys = []
    for d in _offsets(k):
        num = c[:, 1:] + p3 - d                               # o * s
        o = num // s3
        ok = ((num % s3) == 0).all(1) & (num >= 0).all(1) & (o < np.asarray(oshape)).all(1)
        keys.append(cell_key(np.concatenate([c[ok, :1], o[ok]], 1), oshape))
    keys = np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    D, H, W = oshape
    out = np.stack([keys // (D * H * W), keys // (H * W) % D, keys // W % H, keys % W], 1).astype(np.int32)
    return out.reshape(-1, 4), oshape


def neighbours(in_coords, in_shape, out_coords, k, s, p, subm):
    """nbr [n_out, K] int64: input row gathered by output row o at tap t, -1 for none."""
    ic = np.asarray(in_coords).astype(np.int64).reshape(-1, 4)
    oc = np.asarray(out_coords).astype(np.int64).reshape(-1, 4)
    key = cell_key(ic, in_shape)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    offs = _offsets(k)
    nbr = np.full((len(oc), len(offs)), -1, dtype=np.int64)
    if len(ic) == 0 or len(oc) == 0:
        return nbr
    dims = np.asarray(in_shape, np.int64)
    for t, d in enumerate(offs):
        if subm:
            cell = oc[:, 1:] + d - np.asarray(k, np.int64) // 2
        else:
            cell = oc[:, 1:] * np.asarray(s, np.int64) - np.asarray(p, np.int64) + d
        inside = ((cell >= 0) & (cell < dims)).all(1)
        q = cell_key(np.concatenate([oc[:, :1], cell], 1), in_shape)
        pos = np.clip(np.searchsorted(skey, q), 0, len(skey) - 1)
        hit = inside & (skey[pos] == q)
        nbr[hit, t] = order[pos[hit]]
    return nbr


def layer(x, nbr, w, scale=None, shift=None, residual=None, relu=False):
    """x [n, Cin], nbr [n_out, K], w [K, Cin, Cout] -> [n_out, Cout] float64."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    out = np.zeros((nbr.shape[0], w.shape[-1]), dtype=np.float64)
    for t in range(nbr.shape[1]):
        rows = np.nonzero(nbr[:, t] >= 0)[0]
        if len(rows):
            out[rows] += x[nbr[rows, t]] @ w[t]
    if scale is not None:
        out *= np.asarray(scale, np.float64)
    if shift is not None:
        out += np.asarray(shift, np.float64)
    if residual is not None:
        out += np.asarray(residual, np.float64)
    if relu:
        out = np.where(out <= 0.0, 0.0, out)                 # NaN stays NaN
    return out


def layer_norm(x, nbr, w, scale=None, shift=None, residual=None):
    """The abs chain of `layer`: per output element, the sum of the magnitudes of everything summed into it."""
    ab = (lambda a: None if a is None else np.abs(np.asarray(a, np.float64)))
    return layer(ab(x), nbr, ab(w), ab(scale), ab(shift), ab(residual), relu=False)


def sparse_conv(feats, coords, shape, weight, k, s, p, subm, scale=None, shift=None, residual=None, relu=False):
    """One layer: weight [kz, ky, kx, Cin, Cout].  -> dict(out, norm, coords, shape, nbr)."""
    k = [int(v) for v in k]
    if subm:
        ocoords, oshape = np.asarray(coords, np.int32).reshape(-1, 4), [int(v) for v in shape]
    else:
        ocoords, oshape = strided_sites(coords, shape, k, s, p)
    nbr = neighbours(coords, shape, ocoords, k, s, p, subm)
    w = np.asarray(weight, np.float64).reshape(nbr.shape[1], -1, np.shape(weight)[-1])
    return dict(out=layer(feats, nbr, w, scale, shift, residual, relu),
                norm=layer_norm(feats, nbr, w, scale, shift, residual),
                coords=ocoords, shape=oshape, nbr=nbr)


def _np(t):
    return t.detach().cpu().double().numpy()


def _fold(conv, bn):
    """conv bias + eval BatchNorm -> (scale, shift) in float64."""
    scale = _np(bn.weight) / np.sqrt(_np(bn.running_var) + bn.eps)
    shift = _np(bn.bias) - _np(bn.running_mean) * scale
    if conv.bias is not None:
        shift = shift + _np(conv.bias) * scale
    return scale, shift


def encoder_fp64(model, feats, coords, batch, shape):
    """FPNSpMiddleResNetFHD (its ``_stages()``, BN in eval mode) in float64 on sparse sites.

    feats [n, C], coords [n, 4] (b, z, y, x), shape = the sparse shape (D, H, W).  Returns (bev, norm): the last level
    in ``dense_nhwc``'s layout [B, H, W, C*D] (channel c*D + z), and a normaliser in the same layout: the last layer's
    own abs sum (`layer_norm` of that layer on the reference's |input|).

    Not the abs chain through all 21 layers: that multiplies by sum |W| * |scale| per layer and reaches ~1e27 at the
    BEV map of a seeded model whose values are O(10), so any bound relative to it would hold for any output."""
    x = np.asarray(feats, np.float64)
    nx = None
    st = dict(c=np.asarray(coords, np.int32).reshape(-1, 4), shape=[int(v) for v in shape], subm={})

    def conv(m, x, scale, shift, residual=None):
        k, s, p = list(m.kernel_size), list(m.stride), list(m.padding)
        if m.subm:                                        # one table per level and kernel size (spconv's indice_key)
            if tuple(k) not in st["subm"]:
                st["subm"][tuple(k)] = neighbours(st["c"], st["shape"], st["c"], k, s, p, True)
            nbr = st["subm"][tuple(k)]
        else:
            oc, osh = strided_sites(st["c"], st["shape"], k, s, p)
            nbr = neighbours(st["c"], st["shape"], oc, k, s, p, False)
            st.update(c=oc, shape=osh, subm={})
        w = _np(m.weight).reshape(nbr.shape[1], m.in_channels, m.out_channels)
        return layer(x, nbr, w, scale, shift, residual, relu=True), layer_norm(x, nbr, w, scale, shift, residual)

    for seq in model._stages():
        mods = list(seq.children())
        i = 0
        while i < len(mods):
            m = mods[i]
            name = type(m).__name__
            if name in ("SubMConv3d", "SparseConv3d"):
                sc, sh = _fold(m, mods[i + 1])
                x, nx = conv(m, x, sc, sh)
                i += 3
            elif name == "SparseBasicBlock":
                sc1, sh1 = _fold(m.conv1, m.bn1)
                sc2, sh2 = _fold(m.conv2, m.bn2)
                y, _ = conv(m.conv1, x, sc1, sh1)
                x, nx = conv(m.conv2, y, sc2, sh2, residual=x)
                i += 1
            else:
                i += 1
    c, shape = st["c"], st["shape"]
    D, H, W = shape
    C = x.shape[1]
    bev = np.zeros((batch, H, W, C * D), dtype=np.float64)
    nrm = np.zeros_like(bev)
    ch = np.arange(C) * D
    bev[c[:, 0, None], c[:, 2, None], c[:, 3, None], ch[None, :] + c[:, 1, None]] = x
    nrm[c[:, 0, None], c[:, 2, None], c[:, 3, None], ch[None, :] + c[:, 1, None]] = nx
    return bev, nrm
