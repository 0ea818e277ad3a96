"""Dev tool (needs the reference tree; not run by the tests).  Golden vectors for the CenterPoint post-processing, produced
by the reference's own code on the CPU with seeded inputs:

  * ``CenterPointBBoxCoder.decode`` (bevfusion/mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py:121-225) on the
    tensors that ``CenterHead.get_bboxes`` hands it (centerpoint.py:672-698: sigmoid of the heat map, exp of dim, the two
    rot channels), per case and sample: boxes, scores, labels of the survivors;
  * ``circle_nms`` (core/post_processing/box3d_nms.py:180-219) on every case's survivors: kept indices.

THE REFERENCE'S: the coder class and ``circle_nms``, unmodified.  NOT THE REFERENCE'S: the stand-ins that let the two
files import (``mmdet.core.bbox.BaseBBoxCoder`` -> an empty class, ``BBOX_CODERS`` -> a registry that registers nothing,
``numba.jit`` -> identity, ``mmdet3d.ops.iou3d.iou3d_utils.nms_gpu`` -> None), and the three lines of ``get_bboxes`` that
prepare the coder's inputs, restated here with the same torch ops.  ``CenterHead`` itself needs mmcv's ``ConvModule`` and
the CUDA ``nms_gpu``; neither is recorded: the rotated suppression and the convolution graph are pinned by float64 /
torch restatements in the tests, not by this fixture.

Maps are non-square (40 x 24) so that a swapped axis cannot pass.  Only arrays are written:
tests/golden/centerhead.npz.

  python tools/gen_golden_centerhead.py
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden_bevfusion_models as M  # noqa: E402

B, D0, D1 = 2, 40, 24
GEOM = dict(pc_range=[-7.0, -5.0], out_size_factor=4, voxel_size=[0.1, 0.125], post_center_range=[-6.5, -4.5, -3.0, 8.5, 6.5, 3.0])
# name -> (classes, max_num, vel, reg, score_threshold, min_radius of the circle NMS, post_max_size)
CASES = {
    "c1_vel_reg": (1, 50, True, True, 0.1, 0.6, 20),
    "c2_vel_reg": (2, 60, True, True, 0.1, 0.3, 83),
    "c2_novel_reg": (2, 40, False, True, 0.25, 1.0, 10),
    "c1_vel_noreg": (1, 50, True, False, 0.1, 0.175, 83),
}


def import_reference():
    bev = M.BEV
    M._mod("mmdet")
    M._mod("mmdet.core")
    M._mod("mmdet.core.bbox", BaseBBoxCoder=type("BaseBBoxCoder", (), {}))
    M._mod("mmdet.core.bbox.builder", BBOX_CODERS=M._Registry())
    M._pkg("mmdet3d", os.path.join(bev, "mmdet3d"))
    M._pkg("mmdet3d.core", os.path.join(bev, "mmdet3d", "core"))
    M._pkg("mmdet3d.core.bbox", os.path.join(bev, "mmdet3d", "core", "bbox"))
    M._pkg("mmdet3d.core.bbox.coders", os.path.join(bev, "mmdet3d", "core", "bbox", "coders"))
    M._pkg("mmdet3d.core.post_processing", os.path.join(bev, "mmdet3d", "core", "post_processing"))
    M._mod("mmdet3d.ops")
    M._mod("mmdet3d.ops.iou3d")
    M._mod("mmdet3d.ops.iou3d.iou3d_utils", nms_gpu=None, nms_normal_gpu=None)
    M._mod("numba", jit=lambda *a, **k: (lambda fn: fn))
    coder = importlib.import_module("mmdet3d.core.bbox.coders.centerpoint_bbox_coders")
    nms = importlib.import_module("mmdet3d.core.post_processing.box3d_nms")
    return coder.CenterPointBBoxCoder, nms.circle_nms


def main():
    Coder, circle_nms = import_reference()
    out = dict(standin=np.array("BaseBBoxCoder -> empty class; BBOX_CODERS -> no-op registry; numba.jit -> identity; "
                                "nms_gpu -> None; coder inputs prepared as centerpoint.py:672-683"),
               geom=np.array([GEOM["out_size_factor"]] + GEOM["voxel_size"] + GEOM["pc_range"], np.float64),
               post_center_range=np.array(GEOM["post_center_range"], np.float64),
               case_names=np.array(list(CASES)))
    for ci, (name, (ncls, K, has_vel, has_reg, thr, radius, post)) in enumerate(CASES.items()):
        g = torch.Generator().manual_seed(100 + ci)
        heat = torch.randn(B, ncls, D0, D1, generator=g) * 1.5 - 2.0          # logits: a few hundred cells above the threshold
        reg = torch.rand(B, 2, D0, D1, generator=g)
        hei = torch.randn(B, 1, D0, D1, generator=g) * 2.0                     # some heights leave the range
        dim = torch.randn(B, 3, D0, D1, generator=g) * 0.4
        rot = torch.randn(B, 2, D0, D1, generator=g)
        vel = torch.randn(B, 2, D0, D1, generator=g)
        coder = Coder(pc_range=GEOM["pc_range"], out_size_factor=GEOM["out_size_factor"], voxel_size=GEOM["voxel_size"],
                      post_center_range=GEOM["post_center_range"], max_num=K, score_threshold=thr, code_size=9 if has_vel else 7)
        batch_heatmap = heat.sigmoid()                                         # centerpoint.py:672
        batch_dim = torch.exp(dim)                                             # :678 (norm_bbox)
        batch_rots, batch_rotc = rot[:, 0].unsqueeze(1), rot[:, 1].unsqueeze(1)  # :682-683
        temp = coder.decode(batch_heatmap, batch_rots, batch_rotc, hei, batch_dim, vel if has_vel else None,
                            reg=reg if has_reg else None, task_id=0)
        out[f"{name}.cfg"] = np.array([ncls, K, int(has_vel), int(has_reg), thr, radius, post], np.float64)
        for k, v in dict(heat=heat, reg=reg, height=hei, dim=dim, rot=rot, vel=vel).items():
            out[f"{name}.{k}"] = v.numpy()
        out[f"{name}.exp_dim"] = batch_dim.numpy()
        out[f"{name}.sigmoid"] = batch_heatmap.numpy()
        for i in range(B):
            boxes, scores, labels = temp[i]["bboxes"], temp[i]["scores"], temp[i]["labels"]
            out[f"{name}.{i}.bboxes"] = boxes.numpy()
            out[f"{name}.{i}.scores"] = scores.numpy()
            out[f"{name}.{i}.labels"] = labels.numpy()
            dets = torch.cat([boxes[:, [0, 1]], scores.view(-1, 1)], dim=1).numpy()      # centerpoint.py:708-709
            out[f"{name}.{i}.circle_keep"] = np.asarray(circle_nms(dets, radius, post_max_size=post), np.int64)
            print(name, i, "survivors", len(scores), "circle keeps", len(out[f"{name}.{i}.circle_keep"]))
    path = os.path.join(ROOT, "tests", "golden", "centerhead.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
