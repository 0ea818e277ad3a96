"""Dev tool (needs the reference tree; not run by the tests).  Golden vectors for det3d's VFE readers, produced by the
reference's own classes (det3d/models/readers/voxel_encoder.py:13-235) run on the CPU in float32 with seeded parameters
and non-trivial BatchNorm statistics:

  * ``VoxelFeatureExtractor`` and ``VoxelFeatureExtractorV2`` (one and two VFE layers) with ``use_norm`` and
    ``with_distance`` both ways, F = 4 and 5 point features, T = 1, 5, 10 slots, counts from 1 to T;
  * ``SimpleVoxel`` and ``VFEV3_ablation`` on the same voxels.

The voxels lie near (-40, 30, -2): the padded slots, which the reference does not mask in front of the first layer, enter
it as [0..0, -mean, (0)] with a mean far from zero.  The tool asserts that the fixture tells the two readings apart: with
vfe1's max taken over the real slots only (tests/vfe_fp64.py, ``pad_in_max1=False``) the final output of the default
case moves by more than 1e-3 of its magnitude on at least a tenth of the voxels with n < T.

Only inputs, parameters, outputs and the classes' state-dict key lists / shapes are written:
tests/golden/vfe_readers.npz.  The reference file imports det3d pieces through the stand-ins of oracle/ref_import.py;
the forward passes are the reference's code.

  python tools/gen_golden_vfe.py
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import as RI  # noqa: E402
import vfe_fp64 as V  # noqa: E402

M = 36
# (class, num_filters, use_norm, with_distance, F, T); the default sizes once (their 128 x 128 weight is 64 KB)
CASES = [
    ("vfe", [32, 128], True, False, 5, 10),
    ("vfe", [32, 64], False, True, 4, 5),
    ("vfe", [32, 64], True, True, 5, 1),
    ("vfe", [32, 64], False, False, 4, 10),
    ("v2", [32, 64], True, False, 4, 10),
    ("v2", [32, 64], False, True, 5, 5),
    ("v2", [64], True, True, 5, 10),
    ("v2", [64], False, False, 4, 1),
    ("v2", [32], True, False, 5, 5),
]


def import_reference():
    RI.install_standins()
    import det3d.torchie  # noqa: F401
    RI._pkg("det3d.ops", os.path.join(RI.REFERENCE_ROOT, "det3d", "ops"))
    RI._mod("det3d.ops.syncbn", DistributedSyncBN=torch.nn.BatchNorm2d)      # stand-in: unused by the readers
    for pkg in ("det3d.models", "det3d.models.readers"):
        if pkg not in sys.modules:
            RI._pkg(pkg, os.path.join(RI.REFERENCE_ROOT, *pkg.split(".")))
    return importlib.import_module("det3d.models.readers.voxel_encoder")


def seeded_(mod, seed):
    """Every Linear and BatchNorm1d of the reader, in module order: weights ~ N(0, 1/in), non-trivial BN statistics."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight.shape[1] ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
            elif isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    return mod.eval()


def prefixes(kind, filters):
    if kind == "vfe":
        return [("vfe1.linear", "vfe1.norm"), ("vfe2.linear", "vfe2.norm"), ("linear", "norm")]
    return [(f"vfe_layers.{i}.linear", f"vfe_layers.{i}.norm") for i in range(len(filters))] + [("linear", "norm")]


def main():
    ref = import_reference()
    rng = np.random.default_rng(2025)
    store, inputs = {}, {}
    for F in (4, 5):
        for T in (1, 5, 10):
            counts = (np.arange(M) % T) + 1                   # every count from 1 to T
            counts[-1] = T
            vox, num = V.make_case(rng, M, T, F, counts=counts)
            inputs[(F, T)] = (vox, num)
            store[f"voxels_F{F}_T{T}"] = vox
            store[f"num_points_F{F}_T{T}"] = num
    tags = []
    for ci, (kind, filters, use_norm, wd, F, T) in enumerate(CASES):
        tag = f"{kind}_{'x'.join(map(str, filters))}_n{int(use_norm)}_d{int(wd)}_F{F}_T{T}"
        cls = ref.VoxelFeatureExtractor if kind == "vfe" else ref.VoxelFeatureExtractorV2
        mod = seeded_(cls(num_input_features=F, use_norm=use_norm, num_filters=list(filters), with_distance=wd), 300 + ci)
        vox, num = inputs[(F, T)]
        with torch.no_grad():
            out = mod(torch.from_numpy(vox).clone(), torch.from_numpy(num).clone(), None).numpy()
        sd = mod.state_dict()
        params = {k: v.numpy() for k, v in sd.items() if not k.endswith("num_batches_tracked")}
        for k, v in params.items():
            store[f"{tag}.{k}"] = v
        store[f"{tag}.out"] = out
        store[f"{tag}.keys"] = np.array(list(sd))
        store[f"{tag}.shapes"] = np.array([str(tuple(sd[k].shape)) for k in sd])
        store[f"{tag}.config"] = np.array([int(use_norm), int(wd), F, T] + list(filters))
        tags.append(tag)
        # the float64 restatement reproduces the reference (which ran in f32) ...
        layers = V.fold_layers(params, prefixes(kind, filters))
        r64, absum = V.vfe_net(vox, num, layers, wd)
        rel = np.abs(out - r64).max() / np.abs(r64).max()
        assert rel < 1e-5, (tag, rel)
        if ci == 0:
            # ... and the fixture discriminates: masking the padded slots in front of vfe1 moves the output
            wrong, _ = V.vfe_net(vox, num, layers, wd, pad_in_max1=False)
            moved = (np.abs(wrong - out).max(1) > 1e-3 * np.abs(out).max(1))
            partial = num < T
            share = moved[partial].mean()
            assert share >= 0.1, f"{tag}: only {share:.2f} of the voxels with n < T tell the padded-slot rule apart"
            print(f"{tag}: padded-slot rule visible on {share:.2f} of the voxels with n < T")
        print(f"{tag}: out {out.shape}, fp64 restatement within {rel:.2e}")
    for F in (4, 5):
        for T in (1, 5, 10):
            vox, num = inputs[(F, T)]
            f, n = torch.from_numpy(vox), torch.from_numpy(num)
            with torch.no_grad():
                store[f"simple_F{F}_T{T}.out"] = ref.SimpleVoxel(num_input_features=F)(f.clone(), n.clone()).numpy()
                store[f"ablation_F{F}_T{T}.out"] = ref.VFEV3_ablation(num_input_features=F)(f.clone(), n.clone()).numpy()
    for name, cls in (("simple", ref.SimpleVoxel), ("ablation", ref.VFEV3_ablation), ("vfelayer", None)):
        sd = (ref.VFELayer(8, 32) if cls is None else cls()).state_dict()
        store[f"{name}.keys"] = np.array(list(sd), dtype=str)
        store[f"{name}.shapes"] = np.array([str(tuple(sd[k].shape)) for k in sd], dtype=str)
    store["cases"] = np.array(tags)
    out_path = os.path.join(ROOT, "tests", "golden", "vfe_readers.npz")
    np.savez_compressed(out_path, **store)
    print("wrote", out_path, os.path.getsize(out_path), "bytes;", len(tags), "cases of", M, "voxels")


if __name__ == "__main__":
    main()
