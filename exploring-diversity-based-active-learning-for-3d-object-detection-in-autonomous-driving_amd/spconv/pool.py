"""``SparseMaxPool3d`` of the spconv 1.x API on ``al3d_sp_maxpool_f32``."""
import torch

from .. import detector_ops as D
from .. import lib
from ..selector_ops import _dev
from . import ops
from .modules import SparseModule
from .structure import Sites, SparseConvTensor


def _list(v, ndim):
    return [int(x) for x in v] if isinstance(v, (list, tuple)) else [int(v)] * ndim


class SparseMaxPool(SparseModule):
    """Max over the active inputs of every output cell's window; the output cells are a strided conv's (raster order).

    As in spconv the output starts from zero (pool_ops.h:34, maxpool.cc:36), so the result is ``max(0, max over the active
    inputs)`` and a NaN input never wins the comparison.  ``zero_floor=False`` (our extension) gives the true maximum over
    the active inputs instead."""

    def __init__(self, ndim, kernel_size, stride=1, padding=0, dilation=1, subm=False, zero_floor=True):
        super().__init__()
        if ndim != 3:
            raise NotImplementedError(f"al3d.spconv: only the 3-D pool is built (ndim={ndim}): the sparse kernels index "
                                      "(batch, z, y, x) grids")
        self.ndim = ndim
        self.kernel_size, self.stride = _list(kernel_size, ndim), _list(stride, ndim)
        self.padding, self.dilation = _list(padding, ndim), _list(dilation, ndim)
        self.subm, self.zero_floor = subm, zero_floor
        if any(d != 1 for d in self.dilation):
            raise NotImplementedError(f"al3d.spconv: dilation={self.dilation}: the rulebook kernels are built for dilation 1")
        if subm:
            raise NotImplementedError("al3d.spconv: submanifold max pool is not built (no spconv 1.x class selects it)")
        k = self.kernel_size
        if k[0] * k[1] * k[2] > 27:
            raise NotImplementedError(f"al3d.spconv: kernel_size={k} has {k[0] * k[1] * k[2]} taps: the tables hold at most 27")

    def forward(self, input):
        assert isinstance(input, SparseConvTensor)
        if input.features.requires_grad:
            raise NotImplementedError("al3d.spconv is inference only: features.requires_grad is set and no backward kernel "
                                      "exists; detach() the features")
        with torch.no_grad():
            x = input
            feats = _dev(x.features, torch.float32, "features")
            x.check()
            n, batch = x.indices.shape[0], int(x.batch_size)
            shape = [int(v) for v in x.spatial_shape]
            oshape = ops.get_conv_output_size(shape, self.kernel_size, self.stride, self.padding, self.dilation)
            if min(oshape) < 1 or batch * oshape[0] * oshape[1] * oshape[2] >= 2 ** 31:
                raise lib.Al3dError(f"SparseMaxPool3d: output grid {oshape} x batch {batch} must hold between 1 and "
                                    "2^31 - 1 cells")
            if n == 0:
                out_indices, grid_out = x.indices[:0], None
                fout = feats.new_empty((0, feats.shape[1]))
            else:
                grid_out = torch.full((batch * oshape[0] * oshape[1] * oshape[2],), -1, dtype=torch.int32, device=feats.device)
                out_indices = D.sparse_down_sites(x.indices, n, self.kernel_size, self.stride, self.padding, batch, oshape,
                                                  grid_out)
                tab = D.sparse_table(False, out_indices, out_indices.shape[0], batch, shape, x.index_grid(),
                                     self.kernel_size, self.stride, self.padding)
                fout = ops.maxpool(feats, tab, self.zero_floor)
            out = x.on_sites(fout, Sites(out_indices, batch, oshape, checked=True, grid=grid_out), x.indice_dict)
            return out


class SparseMaxPool2d(SparseMaxPool):
    def __init__(self, kernel_size, stride=1, padding=0, dilation=1):
        super().__init__(2, kernel_size, stride, padding, dilation)


class SparseMaxPool3d(SparseMaxPool):
    def __init__(self, kernel_size, stride=1, padding=0, dilation=1, zero_floor=True):
        super().__init__(3, kernel_size, stride, padding, dilation, zero_floor=zero_floor)
