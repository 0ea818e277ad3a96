"""Convolution layers of the spconv 1.x API on this package's sparse kernels (inference only).

Every layer is ONE launch of the encoder's dispatch (``detector_ops.sparse_structure`` / ``sparse_pack`` / ``sparse_table``
/ ``sparse_launch``, so ``AL3D_MATH`` and ``AL3D_SPCONV`` hold here too) over a rulebook that depends on the layer type:

  SubMConv3d             the input sites; ``al3d_sp_subm_table``
  SparseConv3d           every output cell reached by an input; ``al3d_sp_down_sites`` + ``al3d_sp_down_table``
  SparseConvTranspose3d  every output cell i*s - p + d an input i feeds; ``al3d_sp_up_sites`` + ``al3d_sp_up_table``
  SparseInverseConv3d    the paired layer's input sites, row for row; ``al3d_sp_inverse_table`` of the paired table

Strided and transposed outputs are numbered in raster (b, z, y, x) order, i.e. by ascending flat cell index: the order
spconv's CUDA path produces (it sorts the flat output indices), not the first-appearance order of its CPU path."""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import init

from .. import detector_ops as D
from .. import lib
from ..selector_ops import _dev, _ptr, _stream
from ..weight_cache import PackCache
from . import ops
from .modules import SparseModule
from .structure import Sites, SparseConvTensor

# the channel pairs outside the matrix-core set that al3d_sp_conv_f32 is instantiated for; any other runs al3d_sp_conv_any_f32
_VALU_BUILT = {(5, 16), (4, 16)}


class Rulebook:
    """The tables of one layer geometry between two site sets, in the plain and the tiled form, each built on first use
    and then shared by every layer that finds the entry under its ``indice_key``.

    kind "subm" / "conv" / "transposed": ``src`` is the input's ``Sites`` (its index grid is looked up; no feature rows are
    held); kind "inverse": ``src`` is the paired layer's Rulebook.  ``out_sites``: the ``Sites`` of the output rows."""

    def __init__(self, kind, k, stride, pad, src, out_sites):
        self.kind, self.k, self.stride, self.pad, self.src = kind, k, stride, pad, src
        self.out_sites, self.out_indices, self.n_out = out_sites, out_sites.indices, out_sites.indices.shape[0]
        self.n_in = src.n_out if kind == "inverse" else src.indices.shape[0]
        self.tables = {}
        self.inverse = None

    def table(self, tiled):
        tab = self.tables.get(tiled)
        if tab is not None:
            return tab
        src = self.src
        if self.kind == "inverse":
            fwd = next(iter(src.tables.values())) if src.tables else src.table(tiled)
            tab = ops.inverse_table(tiled, fwd, self.n_out)
        else:
            args = (tiled, self.out_indices, self.n_out, int(src.batch_size), [int(v) for v in src.spatial_shape],
                    src.index_grid(), self.k)
            if self.kind == "subm":
                tab = D.sparse_table(*args)
            elif self.kind == "conv":
                tab = D.sparse_table(*args, self.stride, self.pad)
            else:
                tab = ops.up_table(*args, self.stride, self.pad)
        self.tables[tiled] = tab
        return tab


def _tuple3(v, ndim):
    return [int(x) for x in v] if isinstance(v, (list, tuple)) else [int(v)] * ndim


class SparseConvolution(SparseModule):
    """Base of the conv layers: spconv's constructor arguments, ``weight [kz, ky, kx, Cin, Cout]`` and ``bias [Cout]``
    (spconv-1.x state dicts load with ``strict=True``).  The bias travels as the kernel's ``shift``.

    Limits, each a ``NotImplementedError`` that names it: 3-D only, ``dilation == 1``, ``groups == 1``, at most 27 taps,
    no autograd (``features.requires_grad``)."""

    def __init__(self, ndim, in_channels, out_channels, kernel_size=3, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 subm=False, output_padding=0, transposed=False, inverse=False, indice_key=None, fused_bn=False):
        super().__init__()
        if ndim != 3:
            raise NotImplementedError(f"al3d.spconv: only the 3-D layers are built (ndim={ndim}): the sparse kernels index "
                                      "(batch, z, y, x) grids")
        kernel_size, stride, padding = _tuple3(kernel_size, ndim), _tuple3(stride, ndim), _tuple3(padding, ndim)
        dilation, output_padding = _tuple3(dilation, ndim), _tuple3(output_padding, ndim)
        if groups != 1:
            raise NotImplementedError(f"al3d.spconv: groups={groups}: only groups == 1 (as in spconv 1.x)")
        if any(d != 1 for d in dilation):
            raise NotImplementedError(f"al3d.spconv: dilation={dilation}: the rulebook kernels are built for dilation 1")
        if int(np.prod(kernel_size)) > 27:
            raise NotImplementedError(f"al3d.spconv: kernel_size={kernel_size} has {int(np.prod(kernel_size))} taps: the "
                                      "tables and their per-tile tap masks hold at most 27")
        if subm and any(k % 2 == 0 for k in kernel_size):
            raise NotImplementedError(f"al3d.spconv: submanifold kernel_size={kernel_size}: odd sizes only")
        self.ndim, self.in_channels, self.out_channels = ndim, in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = kernel_size, stride, padding, dilation
        self.conv1x1 = int(np.prod(kernel_size)) == 1
        self.transposed, self.inverse, self.output_padding = transposed, inverse, output_padding
        self.groups, self.subm, self.indice_key = groups, subm, indice_key      # fused_bn: spconv's own says "no effect"
        self.weight = nn.Parameter(torch.empty(*kernel_size, in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self._packs = PackCache()
        self.reset_parameters()

    def reset_parameters(self):
        """kaiming-uniform(a = sqrt 5) with fan_in = taps * Cin, the bias uniform in +-1/sqrt(fan_in): nn.Conv3d's rule
        on the [*k, Cin, Cout] layout."""
        fan_in = int(np.prod(self.kernel_size)) * self.in_channels
        bound = math.sqrt(6.0 / ((1.0 + 5.0) * fan_in))
        with torch.no_grad():
            init.uniform_(self.weight, -bound, bound)
            if self.bias is not None:
                init.uniform_(self.bias, -1.0 / math.sqrt(fan_in), 1.0 / math.sqrt(fan_in))

    # ------------------------------------------------------------------ rulebook
    def _geometry(self):
        if self.subm:
            return ("subm", tuple(self.kernel_size))
        return ("transposed" if self.transposed else "conv", tuple(self.kernel_size), tuple(self.stride),
                tuple(self.padding), tuple(self.output_padding) if self.transposed else None)

    def _rulebook(self, x):
        """-> the layer's Rulebook; registers / finds the ``indice_dict`` entry
        ``(out_indices, in_indices, Rulebook, in_spatial_shape, geometry)``."""
        entry = x.find_indice_pair(self.indice_key)
        n = x.indices.shape[0]
        if self.inverse:
            if entry is None:
                raise lib.Al3dError(f"SparseInverseConv3d: no layer has stored indice_key={self.indice_key!r} on this tensor")
            fwd, geom = entry[2], entry[4]
            if tuple(self.kernel_size) != tuple(geom[1]):
                raise lib.Al3dError(f"SparseInverseConv3d: kernel_size={self.kernel_size} but the layer that stored "
                                    f"indice_key={self.indice_key!r} has {list(geom[1])}")
            if fwd.n_out != n:
                raise lib.Al3dError(f"SparseInverseConv3d: indice_key={self.indice_key!r} was stored for {fwd.n_out} output "
                                    f"rows, this tensor has {n}")
            if fwd.inverse is None:
                fwd.inverse = Rulebook("inverse", fwd.k, fwd.stride, fwd.pad, fwd, fwd.src)   # back onto the pair's input sites
            return fwd.inverse
        geom = self._geometry()
        if entry is not None:
            book, have = entry[2], entry[4]
            if have != geom:
                raise lib.Al3dError(f"indice_key={self.indice_key!r} was stored by a layer with geometry {have}, this layer "
                                    f"has {geom}: a rulebook serves one kernel size, stride and padding")
            if book.n_in != n:
                raise lib.Al3dError(f"indice_key={self.indice_key!r} was stored for {book.n_in} input rows, this tensor "
                                    f"has {n}")
            return book
        batch, src = int(x.batch_size), x._sites
        if self.subm:
            book = Rulebook("subm", self.kernel_size, None, None, src, src)
        else:
            oshape = self._out_shape(x)
            if n == 0:
                out_indices, grid_out = x.indices[:0], None
            elif self.transposed:
                out_indices, grid_out = ops.up_sites(x.indices, n, self.kernel_size, self.stride, self.padding, batch, oshape)
            else:
                grid_out = torch.full((batch * oshape[0] * oshape[1] * oshape[2],), -1, dtype=torch.int32,
                                      device=x.indices.device)
                out_indices = D.sparse_down_sites(x.indices, n, self.kernel_size, self.stride, self.padding, batch, oshape,
                                                  grid_out)
            # rows our own site kernels wrote: checked by construction, their index grid comes for free
            book = Rulebook(geom[0], self.kernel_size, self.stride, self.padding, src,
                            Sites(out_indices, batch, oshape, checked=True, grid=grid_out))
        if self.indice_key is not None:
            x.indice_dict[self.indice_key] = (book.out_indices, x.indices, book, x.spatial_shape, geom)
        return book

    def _out_shape(self, x):
        shape = [int(v) for v in x.spatial_shape]
        if self.subm:
            return shape
        if self.transposed:
            out = ops.get_deconv_output_size(shape, self.kernel_size, self.stride, self.padding, self.dilation,
                                             self.output_padding)
        else:
            out = ops.get_conv_output_size(shape, self.kernel_size, self.stride, self.padding, self.dilation)
        if min(out) < 1 or int(x.batch_size) * out[0] * out[1] * out[2] >= 2 ** 31:
            raise lib.Al3dError(f"{type(self).__name__}: output grid {out} x batch {x.batch_size} must hold between 1 and "
                                "2^31 - 1 cells")
        return out

    # ------------------------------------------------------------------ weights
    def _packed(self, dev, name, width, bn):
        """(weights in structure ``name``'s format, scale, shift) for this device, arithmetic and BatchNorm partner; packed
        once per variant and again only when a parameter or buffer of the layer or the partner was written since."""
        def build():
            scale = shift = None
            if bn is not None:
                scale, shift = D.fold_bn(bn, self.bias)
                scale, shift = scale.to(dev), shift.to(dev)
            elif self.bias is not None:
                shift = self.bias.detach().float().to(dev).contiguous()
            w = self.weight.detach().reshape(-1, self.in_channels, self.out_channels).float().to(dev)
            if name == "any":
                return w.contiguous(), scale, shift
            return (*D.sparse_pack(name, w, scale, width), shift)
        return self._packs.get(dev, (self, bn), (D.MATH, name, width, None if bn is None else id(bn)), build)

    # ------------------------------------------------------------------ forward
    def forward(self, input):
        return self.forward_folded(input, None, False)

    def forward_folded(self, input, bn, relu):
        """The layer followed by eval ``bn`` (``BatchNorm1d`` or None) and an optional ReLU, in one launch."""
        assert isinstance(input, SparseConvTensor)
        if input.features.requires_grad:
            raise NotImplementedError("al3d.spconv is inference only: features.requires_grad is set and no backward kernel "
                                      "exists; detach() the features")
        with torch.no_grad():
            return self._forward(input, bn, relu)

    def _forward(self, x, bn, relu):
        feats = _dev(x.features, torch.float32, "features")
        n, cin = feats.shape
        if cin != self.in_channels or n != x.indices.shape[0]:
            raise lib.Al3dError(f"{type(self).__name__}: features {tuple(feats.shape)} do not match in_channels="
                                f"{self.in_channels} and {x.indices.shape[0]} index rows")
        x.check()
        cout, dev = self.out_channels, feats.device
        if self.conv1x1:
            # spconv's quirk: one GEMM over the input rows; the input's indices and shape are returned whatever the stride
            if x._sites.identity is None:
                x._sites.identity = Rulebook("subm", [1, 1, 1], None, None, x._sites, x._sites)
            book = x._sites.identity
        else:
            book = self._rulebook(x)
        K = int(np.prod(self.kernel_size))
        name, width, _ = D.sparse_structure(cin, cout, K, self.subm and not self.conv1x1, False)
        if name is False and (cin, cout) not in _VALU_BUILT:
            name = "any"
        fout = torch.empty((book.n_out, cout), dtype=torch.float32, device=dev)
        if book.n_out:
            w, scale, shift = self._packed(dev, name, width, bn)
            if width != cin:
                feats = torch.nn.functional.pad(feats, (0, width - cin))
            if name == "any":
                tab = book.table(False)
                lib.call("al3d_sp_conv_any_f32", _ptr(feats), _ptr(tab["nbr"]), tab["K"], _ptr(w), cin, cout, _ptr(scale),
                         _ptr(shift), None, 1 if relu else 0, _ptr(fout), tab["n"], _stream())
            else:
                tab = book.table(D.SPARSE[name][2])
                D.sparse_side(name, tab, width, cout)
                D.sparse_launch(name, feats, tab, w, width, cout, scale, shift, None, relu, fout)
        return x.on_sites(fout, book.out_sites, x.indice_dict)


class SparseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias,
                         indice_key=indice_key)


class SubMConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, True,
                         indice_key=indice_key)


class SparseConvTranspose3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias,
                         transposed=True, indice_key=indice_key)


class SparseInverseConv3d(SparseConvolution):
    """Reads the entry a forward layer stored under ``indice_key`` as spconv does: its output indices and shape are that
    layer's INPUT indices and shape (the same rows in the same order), its table that layer's, inverted."""

    def __init__(self, in_channels, out_channels, kernel_size, indice_key, bias=True):
        super().__init__(3, in_channels, out_channels, kernel_size, bias=bias, inverse=True, indice_key=indice_key)


class SparseConv2d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(2, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias,
                         indice_key=indice_key)


class SparseConv4d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(4, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias,
                         indice_key=indice_key)


class SparseConvTranspose2d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(2, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias,
                         transposed=True, indice_key=indice_key)


class SparseInverseConv2d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, indice_key, bias=True):
        super().__init__(2, in_channels, out_channels, kernel_size, bias=bias, inverse=True, indice_key=indice_key)


class SubMConv2d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(2, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, True,
                         indice_key=indice_key)


class SubMConv4d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(4, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, True,
                         indice_key=indice_key)
