"""Containers of the spconv 1.x API: ``SparseModule``, ``SparseSequential``, ``ToDense``, ``RemoveGrid``."""
from collections import OrderedDict

import torch
from torch import nn

from .structure import SparseConvTensor


class SparseModule(nn.Module):
    """Marker base class: a ``SparseSequential`` hands these the ``SparseConvTensor`` itself."""


def _folds(conv, nxt):
    """May ``nxt`` (the module after ``conv``) travel as conv's scale and shift?  An eval-mode BatchNorm1d with statistics."""
    from .conv import SparseConvolution
    return (isinstance(conv, SparseConvolution) and isinstance(nxt, nn.BatchNorm1d) and not nxt.training
            and nxt.running_var is not None)


class SparseSequential(SparseModule):
    """``nn.Sequential`` for sparse tensors: positional modules, one ``OrderedDict``, keyword modules, or ``add``.

    ``SparseModule`` children take the ``SparseConvTensor``; any other ``nn.Module`` acts on its ``.features`` (and is
    skipped on a tensor without rows).  In ``eval()`` a run ``conv -> BatchNorm1d [-> ReLU]`` is ONE launch: the
    BatchNorm is folded (``detector_ops.fold_bn``) into the conv kernel's scale / shift and the ReLU into its epilogue,
    bit-identical to ``detector_ops.sparse_conv_layer`` with that scale and shift.  ``al3d.spconv.FOLD_BN = False`` turns
    the folding off.  The whole forward runs under ``torch.no_grad()``."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], OrderedDict):
            named = list(args[0].items())
        else:
            named = [(str(i), m) for i, m in enumerate(args)]
        for name, module in named + list(kwargs.items()):
            self.add(module, name)

    def __len__(self):
        return len(self._modules)

    def __getitem__(self, idx):
        return list(self._modules.values())[idx]

    def add(self, module, name=None):
        name = str(len(self._modules)) if name is None else name
        if name in self._modules:
            raise KeyError(f"SparseSequential: a module named {name!r} exists")
        self.add_module(name, module)

    def forward(self, x):
        from . import FOLD_BN
        steps = list(self._modules.values())
        with torch.no_grad():                                  # inference only: a plain module's output carries no graph
            at = 0
            while at < len(steps):
                m = steps[at]
                nxt = steps[at + 1:at + 3]
                at += 1
                if FOLD_BN and nxt and _folds(m, nxt[0]):
                    relu = len(nxt) == 2 and type(nxt[1]) is nn.ReLU
                    x = m.forward_folded(x, nxt[0], relu)
                    at += 2 if relu else 1
                elif isinstance(m, SparseModule) or not isinstance(x, SparseConvTensor):
                    x = m(x)
                elif x.features.shape[0]:
                    x.features = m(x.features)
        return x


class ToDense(SparseModule):
    """``SparseConvTensor`` -> dense [B, C, D, H, W]."""

    def forward(self, x):
        return x.dense(channels_first=True)


class RemoveGrid(SparseModule):
    """Forgets spconv's pre-allocated grid buffer (which this package never reads)."""

    def forward(self, x):
        x.grid = None
        return x
