"""Float64 yardsticks of the al3d.spconv layer types, stated from the definitions (numpy + torch.nn.functional on the CPU in
float64), independent of the library.  Built on spconv_fp64.py.

  conv / submanifold   spconv_fp64.sparse_conv
  inverse conv         F.conv_transpose3d of the zero-filled dense map of the rows, w[cin, cout, kz, ky, kx] =
                       W[kz, ky, kx, cin, cout], the PAIRED layer's stride and padding, read at the paired layer's input sites
  transposed conv      the same operator with the layer's own stride, padding and output_padding, read at every cell the
                       enumeration i*s - p + d (d over the kernel offsets, inside the output grid) reaches, ascending cell order
  max pool             numpy max over the active taps of spconv_fp64.neighbours; zero_floor: max(0, .); NaN never wins

Every yardstick returns dict(out, norm, floor, carried, coords, shape):
  norm   the abs chain of spconv_fp64.layer: the same operator on |x| and |W|, plus |bias|; max pool: the max of the taps' |x|
  floor  the f16x3 kernels' absolute term (test_spconv_fp64_gpu.py's header): 2^-36 * the operator on ones and |W|, plus
         `carried`
  carried  the operator on |W| applied to `xfloor`, an absolute error of the input rows handed in (a chain of layers: what
         the input's error can grow to in this layer's output, to first order; max pool: the max over the taps)."""
import numpy as np
import torch
import torch.nn.functional as F

import spconv_fp64 as R

F16_FLOOR = 2.0 ** -36


def _abs(a):
    return None if a is None else np.abs(np.asarray(a, np.float64))


def conv(x, coords, shape, weight, k, s, p, subm, bias=None, xfloor=None):
    r = R.sparse_conv(x, coords, shape, weight, k, s, p, subm, shift=bias)
    w = np.asarray(weight, np.float64).reshape(r["nbr"].shape[1], -1, np.shape(weight)[-1])
    xa = _abs(x)
    r["norm"] = R.layer(xa, r["nbr"], np.abs(w), shift=_abs(bias))
    r["carried"] = 0.0 if xfloor is None else R.layer(xfloor, r["nbr"], np.abs(w))
    r["floor"] = F16_FLOOR * R.layer(np.ones_like(xa), r["nbr"], np.abs(w)) + r["carried"]
    return r


def _dense(x, coords, batch, shape):
    d = torch.zeros((batch, x.shape[1], *[int(v) for v in shape]), dtype=torch.float64)
    c = torch.from_numpy(np.asarray(coords, np.int64).reshape(-1, 4))
    d[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = torch.from_numpy(np.asarray(x, np.float64))
    return d


def _conv_transpose(x, coords, batch, shape, weight, s, p, out_shape, sites):
    """Rows x at coords of grid `shape` -> rows at `sites` of the transposed conv's output grid `out_shape`."""
    k = np.shape(weight)[:3]
    base = [(int(shape[d]) - 1) * int(s[d]) - 2 * int(p[d]) + int(k[d]) for d in range(3)]
    op = [int(out_shape[d]) - base[d] for d in range(3)]
    assert all(0 <= op[d] < max(int(s[d]), 1) or (op[d] == 0) for d in range(3)), (base, out_shape)
    w = torch.from_numpy(np.asarray(weight, np.float64)).permute(3, 4, 0, 1, 2).contiguous()
    y = F.conv_transpose3d(_dense(x, coords, batch, shape), w, stride=tuple(int(v) for v in s),
                           padding=tuple(int(v) for v in p), output_padding=tuple(op))
    assert list(y.shape[2:]) == [int(v) for v in out_shape]
    c = np.asarray(sites, np.int64).reshape(-1, 4)
    return y[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]].numpy()


def _transpose_layer(x, coords, batch, shape, weight, s, p, out_shape, sites, bias, xfloor):
    args = (coords, batch, shape)
    tail = (s, p, out_shape, sites)
    out = _conv_transpose(np.asarray(x, np.float64), *args, np.asarray(weight, np.float64), *tail)
    wa = _abs(weight)
    xa = _abs(x)
    norm = _conv_transpose(xa, *args, wa, *tail)
    carried = 0.0 if xfloor is None else _conv_transpose(xfloor, *args, wa, *tail)
    floor = F16_FLOOR * _conv_transpose(np.ones_like(xa), *args, wa, *tail) + carried
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
        norm = norm + _abs(bias)
    return dict(out=out, norm=norm, floor=floor, carried=carried, coords=np.asarray(sites, np.int32).reshape(-1, 4),
                shape=[int(v) for v in out_shape])


def inverse_conv(x, coords, batch, shape, weight, s, p, pair_coords, pair_shape, bias=None, xfloor=None):
    """x at `coords` (the paired layer's output sites, grid `shape`) -> rows at the paired layer's input sites."""
    return _transpose_layer(x, coords, batch, shape, weight, s, p, pair_shape, pair_coords, bias, xfloor)


def transposed_sites(coords, shape, k, s, p, output_padding):
    """Cells i*s - p + d inside the output grid, ascending cell order -> ([n_out, 4] int32, output shape)."""
    oshape = [(int(shape[d]) - 1) * int(s[d]) - 2 * int(p[d]) + int(k[d]) + int(output_padding[d]) for d in range(3)]
    c = np.asarray(coords).astype(np.int64).reshape(-1, 4)
    keys = []
    for d in R._offsets(k):
        o = c[:, 1:] * np.asarray(s, np.int64) - np.asarray(p, np.int64) + d
        ok = ((o >= 0) & (o < np.asarray(oshape))).all(1)
        keys.append(R.cell_key(np.concatenate([c[ok, :1], o[ok]], 1), oshape))
    keys = np.unique(np.concatenate(keys)) if len(c) else np.zeros(0, np.int64)
    Dz, H, W = oshape
    out = np.stack([keys // (Dz * H * W), keys // (H * W) % Dz, keys // W % H, keys % W], 1).astype(np.int32)
    return out.reshape(-1, 4), oshape


def transposed_conv(x, coords, batch, shape, weight, s, p, output_padding, bias=None, xfloor=None):
    sites, oshape = transposed_sites(coords, shape, np.shape(weight)[:3], s, p, output_padding)
    return _transpose_layer(x, coords, batch, shape, weight, s, p, oshape, sites, bias, xfloor)


def max_pool(x, coords, shape, k, s, p, zero_floor=True, xfloor=None):
    x = np.asarray(x, np.float64)
    sites, oshape = R.strided_sites(coords, shape, k, s, p)
    nbr = R.neighbours(coords, shape, sites, k, s, p, False)

    def pool(v, start):
        out = np.full((len(sites), v.shape[1]), start, dtype=np.float64)
        for t in range(nbr.shape[1]):
            rows = np.nonzero(nbr[:, t] >= 0)[0]
            g = v[nbr[rows, t]]
            out[rows] = np.where(out[rows] < g, g, out[rows])         # a NaN never wins
        return out
    xa = _abs(x)
    carried = pool(np.zeros_like(xa) if xfloor is None else xfloor, 0.0)
    return dict(out=pool(x, 0.0 if zero_floor else -np.inf), norm=pool(xa, 0.0), floor=carried, carried=carried,
                coords=sites, shape=oshape, nbr=nbr)
