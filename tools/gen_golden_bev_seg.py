"""Dev tool (needs the reference tree; not run by the tests).  Golden vectors of the BEV map segmentation head, produced
by the reference's own torch classes on the CPU with seeded parameters:

  * ``BEVGridTransform`` and ``BEVSegmentationHead`` (bevfusion/mmdet3d/models/heads/segm/vanilla.py:47-138): B = 2, a
    non-square 12 x 20 map of 32 channels, K = 6 classes, output grid 20 x 23.  The scopes give a non-integer resampling
    ratio (0.7 and 0.9 input cells per output cell) and output rows / columns that fall partly and wholly outside the map
    (zero padding); both facts are asserted below.

THE REFERENCE'S: the two classes, unmodified, in eval mode.  NOT THE REFERENCE'S: the import stand-ins of
oracle/gen_golden_bevfusion_models.py (imported, not edited) plus a registry stand-in for ``mmdet3d.models.builder.HEADS``.

Only arrays (float32, as the reference computes), the list of state-dict keys and a JSON string of the settings are
written: tests/golden/bev_seg_head.npz.

  python tools/gen_golden_bev_seg.py
"""
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden_bevfusion_models as M  # noqa: E402

HEAD = dict(in_channels=32,
            grid_transform=dict(input_scope=[[-6.0, 6.0, 1.0], [-10.0, 10.0, 1.0]],
                                output_scope=[[-7.5, 6.7, 0.7], [-11.6, 9.0, 0.9]]),
            classes=["drivable_area", "ped_crossing", "walkway", "stop_line", "carpark_area", "divider"], loss="focal")
SHAPE = (2, 32, 12, 20)


def import_reference():
    M.import_reference()
    sys.modules["mmdet3d.models.builder"].HEADS = M._Registry()
    M._pkg("mmdet3d.models.heads", os.path.join(M.BEV, "mmdet3d", "models", "heads"))
    M._pkg("mmdet3d.models.heads.segm", os.path.join(M.BEV, "mmdet3d", "models", "heads", "segm"))
    mod = importlib.import_module("mmdet3d.models.heads.segm.vanilla")
    return mod.BEVGridTransform, mod.BEVSegmentationHead


def padding_facts(in_scope, out_scope, size):
    """(ratio of input cells per output cell, outputs with one neighbour outside, outputs with both outside)."""
    imin, imax, _ = in_scope
    omin, omax, ostep = out_scope
    start = omin + ostep / 2
    n = int(math.ceil((omax - start) / ostep))
    partly = wholly = 0
    for k in range(n):
        pos = (((start + k * ostep - imin) / (imax - imin) * 2 - 1 + 1) * size - 1) / 2
        i0 = math.floor(pos)
        inside = [0 <= i < size for i in (i0, i0 + 1)]
        partly += inside.count(True) == 1
        wholly += inside.count(True) == 0
    return ostep / ((imax - imin) / size), partly, wholly, n


def main():
    BEVGridTransform, BEVSegmentationHead = import_reference()
    gt = HEAD["grid_transform"]
    sizes = []
    for i_s, o_s, size in zip(gt["input_scope"], gt["output_scope"], SHAPE[2:]):
        ratio, partly, wholly, n = padding_facts(i_s, o_s, size)
        assert abs(ratio - round(ratio)) > 0.05, ratio
        assert partly >= 1 and wholly >= 1, (partly, wholly)
        sizes.append(n)
    head = M.seed_(BEVSegmentationHead(**HEAD), 61)
    x = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(23))
    with torch.no_grad():
        grid = head.transform(x)
        prob = head(x)
    assert tuple(grid.shape) == (SHAPE[0], SHAPE[1], *sizes) and tuple(prob.shape) == (SHAPE[0], 6, *sizes)
    assert bool((grid[:, :, 0] == 0).all()) and bool((grid[:, :, :, 0] == 0).all())      # the wholly padded row / column
    store = dict(settings=np.array(json.dumps(dict(head=HEAD, dtype="float32"))), x=x.numpy(), grid=grid.numpy(),
                 prob=prob.numpy(), keys=np.array(sorted(head.state_dict())))
    store.update(M.state_arrays(head, "sd."))
    out = os.path.join(ROOT, "tests", "golden", "bev_seg_head.npz")
    np.savez_compressed(out, **store)
    print("wrote", out, os.path.getsize(out), "bytes;", tuple(grid.shape), tuple(prob.shape))


if __name__ == "__main__":
    main()
