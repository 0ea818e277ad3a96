"""Dev tool (needs the reference tree; not run by the tests).  Golden vectors for two modules of the camera-only BEV
decoder, produced by the reference's own torch classes on the CPU with seeded parameters:

  * ``LSSFPN`` (bevfusion/mmdet3d/models/necks/lss.py:12-65): x1 [1,32,3,5], x2 [1,16,6,10], out_channels 16,
    scale_factor 2 -> [1,16,12,20];
  * ``LSSTransform.get_cam_feats`` (vtransforms/lss.py:61-73 on base.py:21-54): B = 1, N = 2, 16 input channels, D = 5
    depth bins, C = 8 context channels on a 4 x 6 feature map -> depth x context [1,2,5,4,6,8].

THE REFERENCE'S: the two classes, unmodified.  NOT THE REFERENCE'S: the import stand-ins of
oracle/gen_golden_bevfusion_models.py (imported, not edited) plus a registry stand-in for ``mmdet.models.NECKS``.
``GeneralizedResNet`` is not recorded: its ``BasicBlock`` / ``make_res_layer`` come from mmcv, which is not in the reference
tree; the tests pin that block to ``torch.nn`` float64 modules instead.

Only arrays (float32, as the reference computes) and a JSON string of the settings are written:
tests/golden/bevfusion_camera_decoder.npz.

  python tools/gen_golden_camera_decoder.py
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden_bevfusion_models as M  # noqa: E402

FPN = dict(in_indices=[-1, 0], in_channels=[32, 16], out_channels=16, scale_factor=2)
VT = dict(in_channels=16, out_channels=8, image_size=[32, 48], feature_size=[4, 6], xbound=[-8.0, 8.0, 1.0],
          ybound=[-8.0, 8.0, 1.0], zbound=[-10.0, 10.0, 20.0], dbound=[1.0, 6.0, 1.0], downsample=1)


def import_reference():
    M.import_reference()                          # mmcv / mmdet3d stand-ins, vtransforms.base importable
    M._mod("mmdet")
    M._mod("mmdet.models", NECKS=M._Registry(), BACKBONES=M._Registry())
    M._pkg("mmdet3d.models.necks", os.path.join(M.BEV, "mmdet3d", "models", "necks"))
    necks = importlib.import_module("mmdet3d.models.necks.lss")
    vt = importlib.import_module("mmdet3d.models.vtransforms.lss")
    return necks.LSSFPN, vt.LSSTransform


def main():
    LSSFPN, LSSTransform = import_reference()
    store = dict(settings=np.array(json.dumps(dict(fpn=FPN, vtransform=VT, dtype="float32"))))
    g = torch.Generator().manual_seed(21)
    fpn = M.seed_(LSSFPN(**FPN), 51)
    x1, x2 = torch.randn(1, 32, 3, 5, generator=g), torch.randn(1, 16, 6, 10, generator=g)
    with torch.no_grad():
        y = fpn([x2, x1])                         # in_indices [-1, 0]: x1 is the LAST entry, x2 the first
    store.update(fpn_x1=x1.numpy(), fpn_x2=x2.numpy(), fpn_out=y.numpy())
    store.update(M.state_arrays(fpn, "fpn.sd."))
    vt = M.seed_(LSSTransform(**VT), 53)
    x = torch.randn(1, 2, 16, 4, 6, generator=g)
    with torch.no_grad():
        feats = vt.get_cam_feats(x)
    assert tuple(feats.shape) == (1, 2, 5, 4, 6, 8), feats.shape
    store.update(vt_x=x.numpy(), vt_cam_feats=feats.numpy())
    store.update(M.state_arrays(vt, "vt.sd."))
    out = os.path.join(ROOT, "tests", "golden", "bevfusion_camera_decoder.npz")
    np.savez_compressed(out, **store)
    print("wrote", out, os.path.getsize(out), "bytes;", tuple(y.shape), tuple(feats.shape))


if __name__ == "__main__":
    main()
