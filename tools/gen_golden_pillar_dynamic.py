"""Dev tool (needs the reference tree; not run by the tests).  Golden vectors for the dynamic pillar net
(csrc/pillars_dyn.hip, models.DynamicPillarFeatureNet), produced by the reference's own classes run on the CPU with seeded
parameters: det3d ``PillarFeatureNet`` (det3d/models/readers/pillar_encoder.py:17-152) on (b, z, y, x) coordinates and
BEVFusion ``PillarFeatureNet`` (bevfusion/mmdet3d/models/backbones/pillar_encoder.py:20-182) on (b, x, y, z).

The reference tree has no dynamic pillar net.  The clouds are therefore built so that EVERY occupied pillar holds exactly
P = 4 points and the slots are P wide: no padded slot and no truncation exists, so the reference's output on the slots IS
the expected output of a net over all points (asserted: num_points == P everywhere).  The points are stored in a shuffled
order, frames concatenated; the slots hold each pillar's points in ascending point index, as a voxelizer fills them.

Same stand-ins as tools/gen_golden_pointpillars.py (imported read-only from there), labelled in the ``standin`` entry.
Only inputs, the tiny PFN layers' parameters and outputs are written: tests/golden/pillar_dynamic.npz.

  python tools/gen_golden_pillar_dynamic.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_pointpillars as GP  # noqa: E402

P, F = 4, GP.F
NX, NY, B = GP.NX, GP.NY, GP.B         # 48 x 40 x 3, non-square: catches an x / y mix-up
GEOM = GP.GEOM


def make_cloud(rng):
    """-> points [N,F] (frames concatenated, shuffled inside each frame), point_offsets [B+1], voxels [M,P,F] (slots in
    ascending point index), coords [M,4] (b, 0, y, x) in ascending (b, y, x).  Frame 1 is empty; corners and edges of the
    grid are occupied."""
    lo = np.array(GEOM["pc_range"][:2])
    frames, cells, off = [], [], [0]
    for b in range(B):
        if b == 1:
            frames.append(np.zeros((0, F), np.float32))
            off.append(off[-1])
            continue
        fixed = [(0, 0), (NY - 1, NX - 1), (0, NX - 1), (NY - 1, 0), (NY // 2, 0)]
        rest = rng.choice(NY * NX, size=60, replace=False)
        yx = sorted(set(fixed + [divmod(int(c), NX) for c in rest]))
        pts = np.zeros((len(yx) * P, F), np.float32)
        for i, (y, x) in enumerate(yx):
            s = slice(i * P, (i + 1) * P)
            # strictly inside the cell: the voxelizer's floor((p - min) / size) cannot land next door
            pts[s, 0] = lo[0] + (x + rng.uniform(0.1, 0.9, P)) * 0.2
            pts[s, 1] = lo[1] + (y + rng.uniform(0.1, 0.9, P)) * 0.2
            pts[s, 2] = rng.uniform(-4.5, 2.5, P)
            pts[s, 3] = rng.uniform(0, 1, P)
            pts[s, 4] = rng.uniform(0, 0.5, P)
        frames.append(pts[rng.permutation(len(pts))])
        cells += [(b, y, x) for y, x in yx]
        off.append(off[-1] + len(pts))
    points = np.concatenate(frames)
    coords = np.array([[b, 0, y, x] for b, y, x in cells], np.int32)
    # slots: each pillar's points in ascending point index
    vox = np.zeros((len(cells), P, F), np.float32)
    fill = np.zeros(len(cells), np.int64)
    row = {c: i for i, c in enumerate(cells)}
    vs = np.array(GEOM["voxel_size"][:2])
    for b in range(B):
        for p in points[off[b]:off[b + 1]]:
            x, y = np.floor((p[:2].astype(np.float64) - lo) / vs).astype(int)
            r = row[(b, int(y), int(x))]
            vox[r, fill[r]] = p
            fill[r] += 1
    assert (fill == P).all()
    return points, np.array(off, np.int64), vox, fill.astype(np.int32), coords


def main():
    det, bev, _, _ = GP.import_all()
    rng = np.random.default_rng(2025)
    points, off, vox, num, coords = make_cloud(rng)
    assert (num == P).all(), "every occupied pillar must hold exactly P points"
    store = {"standin": np.array(GP.STANDIN), "points": points, "point_offsets": off, "voxels": vox, "num_points": num,
             "coords": coords, "grid": np.array([NX, NY, B]), "voxel_size": np.array(GEOM["voxel_size"]),
             "pc_range": np.array(GEOM["pc_range"])}
    bn = dict(type="BN1d", eps=1e-3, momentum=0.01)
    f, n = torch.from_numpy(vox), torch.from_numpy(num)
    c_det = torch.from_numpy(coords).long()
    c_bev = c_det[:, [0, 3, 2, 1]]
    cases = []
    for filters in ([64], [64, 64]):
        for wd in (False, True):
            tag = f"f{len(filters)}_d{int(wd)}"
            seed = 300 + 10 * len(filters) + int(wd)
            m_det = GP.seeded_pfn_(det.PillarFeatureNet(num_input_features=F, num_filters=filters, with_distance=wd,
                                                        norm_cfg=bn, **GEOM), seed)
            m_bev = GP.seeded_pfn_(bev.PillarFeatureNet(in_channels=F, feat_channels=filters, with_distance=wd,
                                                        voxel_size=GEOM["voxel_size"], point_cloud_range=GEOM["pc_range"],
                                                        norm_cfg=bn), seed)
            with torch.no_grad():
                o_det = m_det(f.clone(), n.clone(), c_det)
                o_bev = m_bev(f.clone(), n.clone(), c_bev)
            for k, v in m_det.state_dict().items():
                if not k.endswith("num_batches_tracked"):
                    store[f"{tag}.{k}"] = v.numpy()
            store[f"{tag}.out_det3d"] = o_det.numpy()
            store[f"{tag}.out_bevfusion"] = o_bev.numpy()
            cases.append(tag)
    store["cases"] = np.array(cases)
    out = os.path.join(ROOT, "tests", "golden", "pillar_dynamic.npz")
    np.savez_compressed(out, **store)
    print("wrote", out, os.path.getsize(out), "bytes;", len(coords), "pillars;", len(points), "points")


if __name__ == "__main__":
    main()
