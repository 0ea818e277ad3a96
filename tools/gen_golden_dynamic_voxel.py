"""Dev tool (needs the reference tree; not run by the tests).  Golden vectors for dynamic voxelization, produced by the
reference's own Python layers run on the CPU:

  * ``Voxelization(max_num_points=-1)`` (bevfusion/mmdet3d/ops/voxel/voxelize.py:77-138) -> per-point (x, y, z);
  * ``DynamicScatter`` with 3- and 4-column ``coors`` and ``dynamic_scatter`` (ops/voxel/scatter_points.py).

Both files import ``.voxel_layer``, the compiled extension, which cannot be built here.  The STAND-IN module registered in
its place holds torch restatements of the two entry points the dynamic path calls:

  * ``dynamic_voxelize``  = src/voxelization_cpu.cpp:8-40: c = floor((p - range_min) / voxel_size) in float32 per axis, the
    whole row -1 when any axis leaves [0, grid);
  * ``dynamic_point_to_voxel_forward`` = src/scatter_points_cuda.cu:183-239: rows with a negative entry masked to -1,
    ``torch.unique(dim=0, sorted=True, return_inverse=True, return_counts=True)``, the -1 row removed, then the reduction.
    The reference reduces with atomicAdd / atomicMax in arrival order; the stand-in adds in float32 one point at a time in
    ascending point index (one of the legal orders), max starts from -inf, mean divides the sum by the count.

The forward code of the two layers is the reference's.  Only inputs and outputs are written:
tests/golden/dynamic_voxel.npz.  No NaN and no zero features are in the inputs (``int c = floor(NaN)`` is undefined in the
reference, and the sign of a zero maximum is arrival-dependent there).

  python tools/gen_golden_dynamic_voxel.py
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import as RI  # noqa: E402

STANDIN = ("mmdet3d.ops.voxel.voxel_layer (compiled extension) -> torch restatements: dynamic_voxelize = "
           "voxelization_cpu.cpp:8-40; dynamic_point_to_voxel_forward = scatter_points_cuda.cu:183-239 with "
           "torch.unique(dim=0, sorted) and a sequential float32 accumulation in ascending point index; "
           "hard_voxelize / dynamic_point_to_voxel_backward unused")
PC_RANGE = [-3.0, -2.0, -1.5, 3.0, 2.0, 1.5]
VOXEL_SIZE = [0.5, 0.4, 0.75]          # grid (x, y, z) = (12, 10, 4): an axis mix-up shows
F = 5


def dynamic_voxelize(points, coors, voxel_size, coors_range, NDim=3):
    vs = torch.tensor(voxel_size, dtype=torch.float32)
    rng = torch.tensor(coors_range, dtype=torch.float32)
    grid = torch.round((rng[3:] - rng[:3]) / vs).to(torch.int32)
    c = torch.floor((points[:, :NDim].float() - rng[:NDim]) / vs[:NDim]).to(torch.int32)
    failed = ((c < 0) | (c >= grid[:NDim])).any(dim=1, keepdim=True)
    coors.copy_(torch.where(failed, torch.full_like(c, -1), c))


def dynamic_point_to_voxel_forward(feats, coors, reduce_type):
    if feats.shape[0] == 0:
        return feats.clone(), coors.clone(), coors.new_empty((0,), dtype=torch.int32), coors.new_empty((0,), dtype=torch.int32)
    clean = coors.masked_fill(coors.lt(0).any(-1, True), -1)
    out_coors, cmap, count = torch.unique(clean, dim=0, sorted=True, return_inverse=True, return_counts=True)
    if bool(out_coors[0, 0] < 0):
        out_coors, count, cmap = out_coors[1:], count[1:], cmap - 1
    cmap, count = cmap.to(torch.int32), count.to(torch.int32)
    red = torch.empty((out_coors.shape[0], feats.shape[1]), dtype=feats.dtype)
    red.fill_(float("-inf") if reduce_type == "max" else 0.0)
    for i in range(feats.shape[0]):
        r = int(cmap[i])
        if r < 0:
            continue
        red[r] = torch.maximum(red[r], feats[i]) if reduce_type == "max" else red[r] + feats[i]
    if reduce_type == "mean":
        red /= count.unsqueeze(-1).to(red.dtype)
    return red, out_coors, cmap, count


def import_reference():
    base = os.path.join(RI.REFERENCE_ROOT, "bevfusion", "mmdet3d", "ops", "voxel")
    for name in ("mmdet3d", "mmdet3d.ops"):
        if name not in sys.modules:
            RI._pkg(name, os.path.join(RI.REFERENCE_ROOT, "bevfusion", *name.split(".")))
    RI._pkg("mmdet3d.ops.voxel", base)
    RI._mod("mmdet3d.ops.voxel.voxel_layer", dynamic_voxelize=dynamic_voxelize, hard_voxelize=None,
            dynamic_point_to_voxel_forward=dynamic_point_to_voxel_forward, dynamic_point_to_voxel_backward=None)
    vox = importlib.import_module("mmdet3d.ops.voxel.voxelize")
    sca = importlib.import_module("mmdet3d.ops.voxel.scatter_points")
    return vox.Voxelization, sca.DynamicScatter, sca.dynamic_scatter


def make_frames(rng):
    """Three frames: uniform points slightly beyond the range (some dropped), a crowded cell, points on cell borders."""
    lo, hi = np.array(PC_RANGE[:3]), np.array(PC_RANGE[3:])
    frames = []
    for n in (700, 450, 620):
        p = np.empty((n, F), np.float32)
        p[:, :3] = rng.uniform(lo - 0.3, hi + 0.3, size=(n, 3))
        p[:, 3] = rng.uniform(0.01, 1.0, n)
        p[:, 4] = rng.uniform(0.01, 0.5, n)
        k = n // 5                                       # a crowded cell and its neighbour, interleaved with the rest
        p[:k:2, :3] = rng.uniform([0.5, 0.4, 0.0], [1.0, 0.8, 0.75], size=(len(p[:k:2]), 3))
        p[1:k:2, :3] = rng.uniform([1.0, 0.4, 0.0], [1.5, 0.8, 0.75], size=(len(p[1:k:2]), 3))
        p[k:k + 12, 0] = lo[0] + 0.5 * np.arange(12)     # exactly on cell borders along x
        p[k + 12, :3] = lo                               # range_min is kept
        p[k + 13, :3] = hi                               # range_max is dropped
        frames.append(p)
    return frames


def main():
    Voxelization, DynamicScatter, dynamic_scatter = import_reference()
    rng = np.random.default_rng(77)
    frames = make_frames(rng)
    vox = Voxelization(VOXEL_SIZE, PC_RANGE, -1).eval()
    store = {"standin": np.array(STANDIN), "pc_range": np.array(PC_RANGE, np.float32),
             "voxel_size": np.array(VOXEL_SIZE, np.float32), "grid": vox.grid_size.numpy(),
             "points": np.concatenate(frames), "offsets": np.cumsum([0] + [len(f) for f in frames]).astype(np.int64)}
    coors = [vox(torch.from_numpy(f)) for f in frames]
    store["point_coords"] = torch.cat(coors).numpy()
    batched = torch.cat([torch.nn.functional.pad(c, (1, 0), value=b) for b, c in enumerate(coors)])
    allpts = torch.from_numpy(store["points"])
    for avg, red in ((True, "mean"), (False, "max")):
        layer = DynamicScatter(VOXEL_SIZE, PC_RANGE, avg)
        f4, c4 = layer(allpts, batched)                  # 4-column coors: the reference's per-frame loop
        store[f"xyz_{red}_feat"], store[f"xyz_{red}_coords"] = f4.numpy(), c4.numpy().astype(np.int32)
        per = [layer(torch.from_numpy(f), c) for f, c in zip(frames, coors)]     # 3-column coors
        assert torch.equal(torch.cat([p[0] for p in per]), f4)
    for red in ("sum", "mean", "max"):
        fz, cz, fx, cx, cnt = [], [], [], [], []
        for b, (f, c) in enumerate(zip(frames, coors)):
            a, o = dynamic_scatter(torch.from_numpy(f), c.flip(-1).contiguous(), red)     # (z, y, x) keys
            fz.append(a)
            cz.append(torch.nn.functional.pad(o, (1, 0), value=b))
            a, o = dynamic_scatter(torch.from_numpy(f), c, red)
            fx.append(a)
            cx.append(torch.nn.functional.pad(o, (1, 0), value=b))
            cnt.append(dynamic_point_to_voxel_forward(torch.from_numpy(f), c.flip(-1).contiguous(), red)[3])
        store[f"zyx_{red}_feat"], store[f"zyx_{red}_coords"] = torch.cat(fz).numpy(), torch.cat(cz).numpy().astype(np.int32)
        store[f"zyx_{red}_counts"] = torch.cat(cnt).numpy()
        if red == "sum":
            store["xyz_sum_feat"], store["xyz_sum_coords"] = torch.cat(fx).numpy(), torch.cat(cx).numpy().astype(np.int32)
        else:
            assert np.array_equal(torch.cat(fx).numpy().view(np.int32), store[f"xyz_{red}_feat"].view(np.int32))
    out = os.path.join(ROOT, "tests", "golden", "dynamic_voxel.npz")
    np.savez_compressed(out, **store)
    print("wrote", out, os.path.getsize(out), "bytes;", len(store["points"]), "points;",
          len(store["zyx_mean_feat"]), "voxels; grid", store["grid"])


if __name__ == "__main__":
    main()
