"""``SparseConvTensor`` of the spconv 1.x API, with the checks and caches our kernels need."""
import numpy as np
import torch

from .. import lib
from ..selector_ops import _dev, _ptr, _stream
from . import ops


class Sites:
    """The site set of a tensor without its features: what the index kernels and the rulebooks hold on to.  Shared by
    every tensor on the same ``indices`` (a submanifold layer's output, an inverse layer's output and its pair's input)."""

    def __init__(self, indices, batch_size, spatial_shape, checked=False, grid=None):
        self.indices, self.batch_size, self.spatial_shape = indices, batch_size, spatial_shape
        self.checked = checked     # indices passed al3d_sp_coords_check (or were written by our own kernels)
        self.grid = grid           # flat [B*D*H*W] i32: row of every active cell, built on first use
        self.identity = None       # rulebook of the kernel-size-1 layers (conv.Rulebook)

    def check(self):
        """Bounds-check ``indices`` (one launch that reads only them, one 4-byte D2H), once per site set."""
        if self.checked:
            return
        dims = [int(v) for v in self.spatial_shape]
        if len(dims) != 3:
            raise NotImplementedError(f"al3d.spconv: 3-D tensors only (spatial_shape has {len(dims)} dimensions)")
        B = int(self.batch_size)
        if B < 1 or min(dims) < 1 or B * dims[0] * dims[1] * dims[2] >= 2 ** 31:
            raise lib.Al3dError(f"SparseConvTensor: batch_size * prod(spatial_shape) = {B} * {dims} must be in [1, 2^31): "
                                "the index grids are addressed with 32-bit cells")
        idx = _dev(self.indices, torch.int32, "indices")
        if idx.dim() != 2 or idx.shape[1] != 4:
            raise lib.Al3dError(f"SparseConvTensor: indices must be [n, 4] (batch, z, y, x), got {tuple(idx.shape)}")
        v = int(ops.coords_status(idx, B, dims).item())
        if v:
            bad = [name for bit, name in enumerate(("batch", "z", "y", "x")) if v >> bit & 1]
            raise lib.Al3dError(f"SparseConvTensor: indices outside batch_size={B}, spatial_shape={dims} in "
                                f"{', '.join(bad)}; no grid kernel was launched")
        self.checked = True

    def index_grid(self):
        """The cached index grid of ``indices`` (checked first)."""
        self.check()
        if self.grid is None:
            self.grid = ops.index_grid(self.indices, self.indices.shape[0], self.batch_size, self.spatial_shape)
        return self.grid


class SparseConvTensor:
    """features [n, C] f32 and indices [n, 4] i32 (batch, z, y, x), both on the device; spatial_shape (D, H, W).

    ``grid`` is spconv's pre-allocated index buffer: accepted and carried along, never read (our index grids belong to
    the site set, ``Sites``, and are cached there).  Before any kernel indexes a grid by ``indices`` they are bounds-checked
    on the device, once per site set (``check``); a row outside ``[0, B) x [0, D) x [0, H) x [0, W)`` raises ``Al3dError``.
    Duplicate rows are NOT detected: as in spconv, the last writer of a cell wins and the other rows become unreachable."""

    def __init__(self, features, indices, spatial_shape, batch_size, grid=None):
        self.features = features
        if indices.dtype != torch.int32:
            indices = indices.to(torch.int32)
        self.indices = indices.contiguous()
        self.spatial_shape = spatial_shape
        self.batch_size = batch_size
        self.indice_dict = {}
        self.grid = grid
        self._sites = Sites(self.indices, batch_size, spatial_shape)

    @property
    def spatial_size(self):
        return np.prod(self.spatial_shape)

    def find_indice_pair(self, key):
        if key is None:
            return None
        return self.indice_dict.get(key)

    def check(self):
        self._sites.check()

    def index_grid(self):
        return self._sites.index_grid()

    def on_sites(self, features, sites, indice_dict):
        """A tensor of this batch on another (or the same) site set, carrying the shared ``indice_dict`` and ``grid``."""
        out = SparseConvTensor(features, sites.indices, sites.spatial_shape, self.batch_size, self.grid)
        out._sites, out.indice_dict = sites, indice_dict
        return out

    def dense(self, channels_first=True):
        """[B, C, D, H, W] (or [B, D, H, W, C]) with zeros at inactive cells, through ``al3d_sp_to_dense_nhwc``."""
        self.check()
        feats = _dev(self.features, torch.float32, "features")
        Dz, H, W = [int(v) for v in self.spatial_shape]
        n, C = feats.shape
        out = torch.zeros((self.batch_size, H, W, C, Dz), dtype=torch.float32, device=feats.device)
        if n:
            lib.call("al3d_sp_to_dense_nhwc", _ptr(feats), _ptr(self.indices), n, C, self.batch_size, Dz, H, W, _ptr(out),
                     _stream())
        if channels_first:
            return out.permute(0, 3, 4, 1, 2).contiguous()
        return out.permute(0, 4, 1, 2, 3).contiguous()
