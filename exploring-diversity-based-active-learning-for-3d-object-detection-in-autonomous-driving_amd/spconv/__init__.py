"""The spconv 1.x inference API on this package's sparse kernels: ``import al3d.spconv as spconv``.

Class names, constructor arguments, parameter names and layouts and the tensor conventions are spconv 1.x's, so model code
written against it (a ``scn.py`` encoder, BEVFusion's ``SparseEncoder``) runs unchanged and its checkpoints load with
``strict=True``.  Inference only: every forward runs under ``torch.no_grad()``.  See DESIGN.md 8f."""
from . import ops
from .conv import (SparseConv2d, SparseConv3d, SparseConv4d, SparseConvolution, SparseConvTranspose2d,
                   SparseConvTranspose3d, SparseInverseConv2d, SparseInverseConv3d, SubMConv2d, SubMConv3d, SubMConv4d)
from .modules import RemoveGrid, SparseModule, SparseSequential, ToDense
from .pool import SparseMaxPool, SparseMaxPool2d, SparseMaxPool3d
from .structure import SparseConvTensor

# eval-mode ``conv -> BatchNorm1d [-> ReLU]`` runs inside a SparseSequential are one launch; False: three modules
FOLD_BN = True

__all__ = ["FOLD_BN", "RemoveGrid", "SparseConv2d", "SparseConv3d", "SparseConv4d", "SparseConvTensor",
           "SparseConvTranspose2d", "SparseConvTranspose3d", "SparseConvolution", "SparseInverseConv2d",
           "SparseInverseConv3d", "SparseMaxPool", "SparseMaxPool2d", "SparseMaxPool3d", "SparseModule", "SparseSequential",
           "SubMConv2d", "SubMConv3d", "SubMConv4d", "ToDense", "ops"]
