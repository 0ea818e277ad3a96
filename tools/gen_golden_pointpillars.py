"""Dev tool (needs the reference tree; not run by the tests).  Golden vectors for the PointPillars encoder, produced by the
reference's own classes run on the CPU with seeded parameters:

  * det3d ``PillarFeatureNet`` / ``PointPillarsScatter`` (det3d/models/readers/pillar_encoder.py:17-211) on (b, z, y, x)
    coordinates;
  * BEVFusion ``PillarFeatureNet`` / ``PointPillarsScatter`` (bevfusion/mmdet3d/models/backbones/pillar_encoder.py:20-240)
    on (b, x, y, z) coordinates;
  * BEVFusion ``SECOND`` + ``SECONDFPN`` with the pointpillars.yaml decoder settings (64/128/256 channels, strides 2/2/2,
    3/5/5 layers; upsample strides 0.5/1/2, 3 x 128) on the BEVFusion scatter's canvas.

The reference files import mmcv / mmdet / det3d pieces that are absent here (ordinary ModuleNotFoundErrors).  The
stand-ins are the FACTORY STAND-INS of oracle/gen_golden_bevfusion_second.py (imported read-only), plus
``build_norm_layer(BN1d)`` -> ``nn.BatchNorm1d(eps, momentum)``, an empty ``mmdet3d.models.builder`` and det3d's syncbn ->
``nn.BatchNorm2d``; labelled in the fixture's ``standin`` entry.  The forward passes are the reference's code.  Only
inputs, parameters of the tiny PFN layers and outputs are written: tests/golden/pointpillars.npz.

  python tools/gen_golden_pointpillars.py
"""
import importlib
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden_bevfusion_second as S  # noqa: E402
import ref_import as RI  # noqa: E402

STANDIN = S.STANDIN + "; build_norm_layer(BN1d) -> nn.BatchNorm1d(eps, momentum); det3d syncbn -> nn.BatchNorm2d; " \
                      "mmdet3d.models.builder.build_backbone unused"
P, F = 20, 5
NX, NY, B = 48, 40, 3                 # non-square: catches an x / y mix-up
GEOM = dict(voxel_size=[0.2, 0.2, 8], pc_range=[-4.8, -4.0, -5.0, 4.8, 4.0, 3.0])


def build_norm_layer(cfg, num_features, postfix=""):
    cfg = dict(cfg)
    t = cfg.pop("type")
    cfg.pop("requires_grad", None)
    if t == "BN1d":
        return "bn" + str(postfix), nn.BatchNorm1d(num_features, **cfg)
    return S.build_norm_layer(dict(cfg, type=t), num_features, postfix)


def import_all():
    SECOND, SECONDFPN, _ = S.import_reference()
    sys.modules["mmcv.cnn"].build_norm_layer = build_norm_layer
    S._mod("mmdet3d.models.builder", build_backbone=None)
    bev = importlib.import_module("mmdet3d.models.backbones.pillar_encoder")
    RI.install_standins()
    import det3d.torchie  # noqa: F401
    RI._pkg("det3d.ops", os.path.join(RI.REFERENCE_ROOT, "det3d", "ops"))
    RI._mod("det3d.ops.syncbn", DistributedSyncBN=nn.BatchNorm2d)
    for pkg in ("det3d.models", "det3d.models.readers"):
        RI._pkg(pkg, os.path.join(RI.REFERENCE_ROOT, *pkg.split(".")))
    det = importlib.import_module("det3d.models.readers.pillar_encoder")
    return det, bev, SECOND, SECONDFPN


def make_pillars(rng):
    """Pillars of B frames (frame 1 empty) in this build's (b, z, y, x): counts 1, several, exactly P and beyond P
    (num_points_raw keeps those; the voxelizer clips them to P), grid corners and edges included."""
    cells = []
    for b in (0, 2):
        fixed = [(0, 0), (NY - 1, NX - 1), (0, NX - 1), (NY - 1, 0), (NY // 2, 0)]
        rest = rng.choice(NY * NX, size=60, replace=False)
        pts = fixed + [divmod(int(c), NX) for c in rest if divmod(int(c), NX) not in fixed]
        cells += [(b, y, x) for y, x in pts]
    M = len(cells)
    coords = np.array([[b, 0, y, x] for b, y, x in cells], np.int32)
    raw = rng.integers(1, P + 1, size=M)
    raw[:6] = [1, 2, P, P + 3, 7, P + 11]
    raw[40:43] = [P, 1, P + 1]
    vox = np.zeros((M, P, F), np.float32)
    lo = np.array(GEOM["pc_range"][:2])
    for i, (b, y, x) in enumerate(cells):
        k = min(int(raw[i]), P)
        vox[i, :k, 0] = lo[0] + (x + rng.uniform(0, 1, k)) * 0.2
        vox[i, :k, 1] = lo[1] + (y + rng.uniform(0, 1, k)) * 0.2
        vox[i, :k, 2] = rng.uniform(-5, 3, k)
        vox[i, :k, 3] = rng.uniform(0, 1, k)
        vox[i, :k, 4] = rng.uniform(0, 0.5, k)
    return vox, raw.astype(np.int32), coords


def seeded_pfn_(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in mod.pfn_layers:
            w = p.linear.weight
            w.copy_(torch.randn(w.shape, generator=g) / w.shape[1] ** 0.5)
            n = p.norm
            n.weight.copy_(torch.rand(n.weight.shape, generator=g) + 0.5)
            n.bias.copy_(torch.randn(n.bias.shape, generator=g) * 0.3)
            n.running_mean.copy_(torch.randn(n.running_mean.shape, generator=g) * 0.3)
            n.running_var.copy_(torch.rand(n.running_var.shape, generator=g) + 0.5)
    return mod.eval()


def main():
    det, bev, SECOND, SECONDFPN = import_all()
    rng = np.random.default_rng(2024)
    vox, raw, coords = make_pillars(rng)
    num = np.minimum(raw, P).astype(np.int32)
    store = {"standin": np.array(STANDIN), "voxels": vox, "num_points_raw": raw, "coords": coords,
             "grid": np.array([NX, NY, B]), "voxel_size": np.array(GEOM["voxel_size"]),
             "pc_range": np.array(GEOM["pc_range"])}
    bn = dict(type="BN1d", eps=1e-3, momentum=0.01)
    f, n = torch.from_numpy(vox), torch.from_numpy(num)
    c_det = torch.from_numpy(coords).long()
    c_bev = c_det[:, [0, 3, 2, 1]]
    cases = []
    for filters in ([64], [64, 64]):
        for wd in (False, True):
            tag = f"f{len(filters)}_d{int(wd)}"
            seed = 100 + 10 * len(filters) + int(wd)
            m_det = seeded_pfn_(det.PillarFeatureNet(num_input_features=F, num_filters=filters, with_distance=wd,
                                                     norm_cfg=bn, **GEOM), seed)
            m_bev = seeded_pfn_(bev.PillarFeatureNet(in_channels=F, feat_channels=filters, with_distance=wd,
                                                     voxel_size=GEOM["voxel_size"],
                                                     point_cloud_range=GEOM["pc_range"], norm_cfg=bn), seed)
            with torch.no_grad():
                o_det = m_det(f.clone(), n.clone(), c_det)
                o_bev = m_bev(f.clone(), n.clone(), c_bev)
            for k, v in m_det.state_dict().items():
                if not k.endswith("num_batches_tracked"):
                    store[f"{tag}.{k}"] = v.numpy()
            store[f"{tag}.out_det3d"] = o_det.numpy()
            store[f"{tag}.out_bevfusion"] = o_bev.numpy()
            cases.append(tag)
            if filters == [64, 64] and not wd:
                with torch.no_grad():
                    cd = det.PointPillarsScatter(num_input_features=64)(o_det, c_det, B, [NX, NY, 1])
                    cb = bev.PointPillarsScatter(in_channels=64, output_shape=[NX, NY])(o_bev, c_bev, B)
                store["canvas_det3d"] = cd.numpy()          # [B, C, ny, nx]
                store["canvas_bevfusion"] = cb.numpy()      # [B, C, nx, ny]
                bn2 = dict(type="BN", eps=1.0e-3, momentum=0.01)
                backbone, d0 = S.seeded_state_(SECOND(in_channels=64, out_channels=[64, 128, 256], layer_nums=[3, 5, 5],
                                                      layer_strides=[2, 2, 2], norm_cfg=bn2,
                                                      conv_cfg=dict(type="Conv2d", bias=False)), 11)
                neck, d1 = S.seeded_state_(SECONDFPN(in_channels=[64, 128, 256], out_channels=[128, 128, 128],
                                                     upsample_strides=[0.5, 1, 2], norm_cfg=bn2,
                                                     upsample_cfg=dict(type="deconv", bias=False),
                                                     use_conv_for_no_stride=True), 12)
                with torch.no_grad():
                    dec = neck(backbone(cb))[0]
                store["decoder_out"] = dec.numpy()            # [B, 384, nx / 4, ny / 4]
                store["decoder_seeds"] = np.array([11, 12])
                store["decoder_digest"] = np.array([d0, d1])
                for part, mod in (("backbone", backbone), ("neck", neck)):
                    sd = mod.state_dict()
                    store[f"keys_{part}"] = np.array(sorted(sd))
                    store[f"shapes_{part}"] = np.array([str(tuple(sd[k].shape)) for k in sorted(sd)])
    store["cases"] = np.array(cases)
    store["pfn_keys_bevfusion"] = np.array(list(m_bev.state_dict()))
    out = os.path.join(ROOT, "tests", "golden", "pointpillars.npz")
    np.savez_compressed(out, **store)
    print("wrote", out, os.path.getsize(out), "bytes;", len(coords), "pillars; decoder", tuple(dec.shape))


if __name__ == "__main__":
    main()
