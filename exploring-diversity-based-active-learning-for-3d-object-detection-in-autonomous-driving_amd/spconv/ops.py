"""Output-size formulas of the spconv 1.x API and the device-side index work of ``al3d.spconv``.

Every rulebook here is the output-major, tap-major table the conv kernels of this package read (``nbr[k][o]`` = input row or
-1; ``detector_ops.sparse_table``), in the plain form ([K, max(n, 1)]) or the tiled one (pitched, with per-tile tap masks),
whichever the layer's kernel structure takes."""
import torch

from .. import detector_ops as D
from .. import lib
from ..selector_ops import _ptr, _stream


def get_conv_output_size(input_size, kernel_size, stride, padding, dilation):
    """Per dimension ``(in + 2 p - d (k - 1) - 1) // s + 1``; a kernel size of -1 gives 1."""
    return [1 if kernel_size[i] == -1 else
            (input_size[i] + 2 * padding[i] - dilation[i] * (kernel_size[i] - 1) - 1) // stride[i] + 1
            for i in range(len(input_size))]


def get_deconv_output_size(input_size, kernel_size, stride, padding, dilation, output_padding):
    """Per dimension ``(in - 1) s - 2 p + k + output_padding`` (the dilation does not enter, as in spconv 1.x)."""
    if any(k == -1 for k in kernel_size):
        raise ValueError(f"get_deconv_output_size: kernel_size={list(kernel_size)}: a transposed conv has no -1 (whole-axis) kernel")
    return [(input_size[i] - 1) * stride[i] - 2 * padding[i] + kernel_size[i] + output_padding[i]
            for i in range(len(input_size))]


def coords_status(indices, batch_size, spatial_shape):
    """One launch of ``al3d_sp_coords_check`` over indices [n, 4] i32 -> the device status word (0 = every row inside)."""
    status = torch.empty(1, dtype=torch.int32, device=indices.device)
    lib.call("al3d_sp_coords_check", _ptr(indices), indices.shape[0], int(batch_size), *[int(v) for v in spatial_shape],
             _ptr(status), _stream())
    return status


def index_grid(indices, n, batch_size, spatial_shape):
    """Flat [B*D*H*W] i32 grid: row of every active cell, -1 elsewhere."""
    dims = [int(v) for v in spatial_shape]
    grid = torch.full((int(batch_size) * dims[0] * dims[1] * dims[2],), -1, dtype=torch.int32, device=indices.device)
    lib.call("al3d_sp_scatter_index", _ptr(indices), n, int(batch_size), *dims, _ptr(grid), 1, _stream())
    return grid


def up_sites(coords, n, k, stride, pad, batch, odims):
    """Output sites of a transposed conv over the n input sites ``coords`` (input i feeds the cells i*s - p + d), numbered in
    raster (b, z, y, x) order.  One small D2H.  -> (coords_out [n_out, 4] i32, grid_out: their index grid)"""
    dev = coords.device
    odims = [int(v) for v in odims]
    cells = batch * odims[0] * odims[1] * odims[2]
    cap = min(n * int(k[0]) * int(k[1]) * int(k[2]), cells)
    grid_out = torch.full((cells,), -1, dtype=torch.int32, device=dev)
    out = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.load().al3d_sp_up_sites_workspace_bytes(batch, *odims), dtype=torch.uint8, device=dev)
    lib.call("al3d_sp_up_sites", _ptr(coords), n, D._i3(k), D._i3(stride), D._i3(pad), batch, *odims, _ptr(grid_out), _ptr(out),
             _ptr(counter), cap, _ptr(ws), _stream())
    return out[:int(counter.item())], grid_out


def _empty_table(tiled, n, K, dev):
    if tiled:
        pitch = lib.load().al3d_sp_table_pitch(n)
        nbr = torch.empty((K, pitch), dtype=torch.int32, device=dev)
        tmask = torch.empty((pitch // 32,), dtype=torch.int32, device=dev)
        return nbr, tmask, (_ptr(nbr), pitch, _ptr(tmask))
    nbr = torch.empty((K, max(n, 1)), dtype=torch.int32, device=dev)
    return nbr, None, (_ptr(nbr),)


def up_table(tiled, coords_out, n_out, batch, dims, grid, k, stride, pad):
    """``detector_ops.sparse_table`` for a transposed conv: dims and grid are the input level's."""
    K = int(k[0]) * int(k[1]) * int(k[2])
    nbr, tmask, out = _empty_table(tiled, n_out, K, coords_out.device)
    lib.call("al3d_sp_up_table" + ("_tiles" if tiled else ""), _ptr(coords_out), n_out, D._i3(k), D._i3(stride), D._i3(pad),
             batch, *[int(v) for v in dims], _ptr(grid), *out, _stream())
    return dict(nbr=nbr, n=n_out, K=K, tmask=tmask)


def inverse_table(tiled, fwd, n_in):
    """The table of the inverse conv paired with the layer whose table is ``fwd`` (either form) over n_in input rows."""
    K = fwd["K"]
    nbr, tmask, out = _empty_table(tiled, n_in, K, fwd["nbr"].device)
    lib.call("al3d_sp_inverse_table" + ("_tiles" if tiled else ""), _ptr(fwd["nbr"]), fwd["nbr"].shape[1], K, fwd["n"], n_in,
             *out, _stream())
    return dict(nbr=nbr, n=n_in, K=K, tmask=tmask)


def maxpool(feats, tab, zero_floor):
    """[n_out, C] = max over the active taps of the plain table ``tab``."""
    out = torch.empty((tab["n"], feats.shape[1]), dtype=torch.float32, device=feats.device)
    if tab["n"]:
        lib.call("al3d_sp_maxpool_f32", _ptr(feats), _ptr(tab["nbr"]), tab["nbr"].shape[1], tab["K"], feats.shape[1], tab["n"],
                 1 if zero_floor else 0, _ptr(out), _stream())
    return out
