"""CPU suite: ``TransFusionHead._decode`` (host torch on a few hundred proposals) against the reference's own
``TransFusionBBoxCoder.decode(..., filter=True)`` (bevfusion/mmdet3d/core/bbox/coders/transfusion_bbox_coder.py:39-123), run by
oracle/gen_golden_bevfusion_models.py on seeded inputs: boxes, scores and labels of every surviving proposal, bit for bit.

The box sizes are ``exp`` of the raw outputs, and torch's float32 ``exp`` on the CPU is MKL's vector math, whose last bit
depends on the code path MKL picks for the processor (the golden's generator ran the AVX-512 path of an Intel part; an AMD
part rounds a few elements the other way).  Where this host's ``exp`` of the stored input differs from the golden's, the
golden value must be within 1 ulp of it, and the expected box then holds the reference's expressions evaluated on this
host's ``exp`` (size, and the bottom height derived from it); every other value is the golden's, bit for bit."""
import os
import types

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bevfusion_transfusion_decode.npz")


def _expected_boxes(z, i):
    """Golden boxes of sample i with the exp-derived entries re-evaluated on this host's exp where it rounds differently."""
    gold = torch.from_numpy(z[f"out{i}.bboxes"]).clone()
    vel = torch.from_numpy(z["vel"][i]).T                                  # (proposals, 2): copied into the box unchanged
    assert len(torch.unique(vel, dim=0)) == len(vel)
    idx, p = [], 0                                                          # surviving proposals, in proposal order
    for row in gold:
        while not torch.equal(vel[p], row[7:9]):
            p += 1
        idx.append(p)
        p += 1
    dim = torch.from_numpy(z["dim"])
    host = torch.stack([dim[:, k, :].exp() for k in range(3)], 1)[i, :, idx].T     # the coder's own per-channel exp
    ulps = (host.view(torch.int32).long() - gold[:, 3:6].view(torch.int32).long()).abs()
    assert int(ulps.max()) <= 1, "the golden's exp is more than 1 ulp from this host's"
    differs = ulps != 0
    gold[:, 3:6] = torch.where(differs, host, gold[:, 3:6])
    rows = differs[:, 2]
    height = torch.from_numpy(z["height"])[i, 0, idx]
    gold[rows, 2] = height[rows] - host[rows, 2] * 0.5
    return gold


def test_transfusion_decode_equals_the_reference_coder():
    from al3d.models.transfusion_head import TransFusionHead
    z = np.load(GOLD)
    t = lambda k: torch.from_numpy(z[k])                                 # noqa: E731
    coder = dict(pc_range=[-54.0, -54.0], voxel_size=[0.075, 0.075], out_size_factor=8,
                 post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], score_threshold=float(z["score_threshold"][0]))
    got = TransFusionHead._decode(types.SimpleNamespace(bbox_coder=coder), t("heat"), t("rot"), t("dim"), t("center"),
                                  t("height"), t("vel"))
    assert len(got) == 2
    kept = 0
    for i, r in enumerate(got):
        assert torch.equal(r["bboxes"], _expected_boxes(z, i)) and torch.equal(r["scores"], t(f"out{i}.scores"))
        assert torch.equal(r["labels"], t(f"out{i}.labels"))
        kept += len(r["scores"])
    assert 0 < kept < 2 * z["heat"].shape[2]                              # the filters removed something, not everything
