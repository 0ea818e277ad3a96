"""The one runner of a folded dense convolution: Conv2d(s) [+ BatchNorm2d] [+ ReLU] on channels-last maps."""
from torch.nn import functional as F

from .. import detector_ops as D
from ..weight_cache import PackCache


class FoldedConv:
    """``pairs``: the ``(conv, bn or None)`` layers reading the same input (more than one: their outputs side by side in
    one launch); ``fold``: ``detector_ops.fold_conv_bn``'s options.  Folded and packed for the dense conv dispatch on first
    use, once per arithmetic / structure, and again after any of their parameters or buffers is written.

    Not an ``nn.Module``: it holds references to the owner's layers, so the state dict keeps the owner's keys only.

    Input channels are always zero-padded to a multiple of 16 (weights at pack time, the map per call), which the
    matrix-core kernels need.  There is no geometry-less plain-format path for other channel counts: every layer this
    build ships with Conv + BN + ReLU only (the view transform's ``downsample``, ``ConvFuser``) has Cin % 16 == 0, where
    padding is a no-op and the launch is the same one."""

    def __init__(self, pairs, relu=True, **fold):
        self.pairs = list(pairs)
        self.sources = [m for pair in self.pairs for m in pair]
        conv = self.pairs[0][0]
        self.geom = (conv.kernel_size[0], conv.stride[0], conv.padding[0])
        self.relu, self.fold = relu, fold
        self.cache = PackCache()

    def packed(self, device):
        """(weights, scale, shift) on ``device`` under the current ``MATH`` / ``DENSE``."""
        def build():
            w, scale, shift = D.fold_conv_bn(self.pairs, pad_cin=True, **self.fold)
            w, scale = D.pack_dense(w.to(device), scale.to(device), *self.geom)
            return w, scale, shift.to(device)
        return self.cache.get(device, self.sources, (D.MATH, D.DENSE), build)

    def kind(self, device):
        """The structure (``detector_ops.DENSE_KINDS``) the layer runs on: what pair-pixel decisions read."""
        return D.dense_kind(self.packed(device)[0])

    def __call__(self, x, out=None, coff=0, gap=None, io=0):
        w, scale, shift = self.packed(x.device)
        pad = -x.shape[-1] % 16
        if pad:
            x = F.pad(x, (0, pad))
        return D.conv2d_nhwc(x.contiguous(), w, scale, shift, *self.geom, self.relu, out=out, coff=coff, gap=gap, io=io)
