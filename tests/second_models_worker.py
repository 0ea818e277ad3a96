"""Shared case and child process of tests/test_second_models_gpu.py: SpMiddleFHD and SpMiddleResNetFHD on a small grid
(input_shape [96, 88, 40], batch 2 with an empty second frame, 2,000 random voxels) against spconv_fp64.encoder_fp64,
normalised as tests/test_spconv_fp64_gpu.py normalises the whole encoder (the last layer's own abs sum).  Run as a
program it prints one JSON line with the error of both encoders under the AL3D_MATH of the environment."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

INPUT_SHAPE = [96, 88, 40]                   # (nx, ny, nz); the sparse shape is [41, 88, 96]
BATCH = 2
ENCODERS = {"SpMiddleResNetFHD": 5, "SpMiddleFHD": 128}      # name -> input channels (the example configs')


def make_inputs(cin, n=2000, seed=7):
    """feats [n, cin] f32, coords [n, 4] i32 (b, z, y, x) in random row order, every voxel in frame 0."""
    from test_detector_oracle import random_sparse
    rng = np.random.default_rng(seed + cin)
    feats, coords = random_sparse(rng, 1, [41, 88, 96], n, cin)
    return feats, coords


def build(name, seed=3):
    from al3d import synthetic
    from al3d.models import build_backbone
    m = build_backbone(dict(type=name, num_input_features=ENCODERS[name], ds_factor=8, norm_cfg=None))
    synthetic.seeded_init_(m, seed=seed)
    return m.eval()


_REF = {}


def reference(name):
    """(ref, norm) of encoder_fp64, computed once per process."""
    import spconv_fp64 as R
    if name not in _REF:
        feats, coords = make_inputs(ENCODERS[name])
        _REF[name] = R.encoder_fp64(build(name), feats, coords, BATCH, [41, 88, 96])
    return _REF[name]


def encoder_error(name, dev="cuda:0"):
    """max |got - ref| / norm over the cells with a site; cells without one must be exactly 0."""
    feats, coords = make_inputs(ENCODERS[name])
    model = build(name).to(dev)
    with torch.no_grad():
        got = model(torch.from_numpy(feats).to(dev), torch.from_numpy(coords).to(dev), BATCH, INPUT_SHAPE)
    got = got.cpu().double().numpy()
    ref, norm = reference(name)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    live = norm > 0
    return dict(e=float((np.abs(got - ref)[live] / norm[live]).max()), zero=bool((got[~live] == 0).all()),
                shape=list(got.shape), sites=int(live.sum()))


def main():
    from al3d import detector_ops as D
    out = dict(math=D.MATH)
    for name in ENCODERS:
        out[name] = encoder_error(name)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
