"""Child process of tests/test_camera_decoder_gpu.py: one BasicBlock with a downsample shortcut (8 x 8, 32 -> 64, stride 2)
under the AL3D_MATH of the environment, against the float64 yardstick.  Prints one JSON line: the arithmetic, the
error as a fraction of the block's abs-chain normaliser, whether the output is finite, and whether the two-step path
writes a channel window of a wider map correctly and refuses one that does not fit."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main():
    import camera_decoder_fp64 as Y
    from test_camera_decoder_cpu import seed_module_
    from al3d import detector_ops as D
    from al3d.models.bevfusion_camera_only import make_res_layer
    dev = "cuda:0"
    blk = seed_module_(make_res_layer(32, 64, 1, stride=2), 5)
    x = torch.randn(2, 32, 8, 8, generator=torch.Generator().manual_seed(6))
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    ref = Y.basic_block64(x.double(), sd, "0.", 2)
    norm = Y.basic_block64(x.double().abs(), Y.abs_state(sd), "0.", 2)      # the abs chain of the block
    with torch.no_grad():
        got = blk.to(dev).eval()(x.permute(0, 2, 3, 1).contiguous().to(dev))
    torch.cuda.synchronize()
    got = got.cpu().double().permute(0, 3, 1, 2)
    # the generic path writing into a window of a wider map, and its window check
    from al3d import lib
    c = torch.randn(1, 4, 4, 32, generator=torch.Generator().manual_seed(7)).to(dev)
    r = torch.randn(1, 4, 4, 32, generator=torch.Generator().manual_seed(8)).to(dev)
    w, sc = D.pack_res3x3((torch.randn(32, 9, 32, generator=torch.Generator().manual_seed(9)) / 17.0).to(dev), None)
    plain = D.conv3x3_res_nhwc(c, w, sc, None, r)
    wide = torch.full((1, 4, 4, 44), -5.0, device=dev)
    D.conv3x3_res_nhwc(c, w, sc, None, r, out=wide, coff=8)
    window = bool(torch.equal(wide[..., 8:40], plain) and (wide[..., :8] == -5.0).all() and (wide[..., 40:] == -5.0).all())
    refused = False
    small = torch.full((1, 4, 4, 36), -5.0, device=dev)
    try:
        D.conv3x3_res_nhwc(c, w, sc, None, r, out=small, coff=8)
    except lib.Al3dError:
        refused = bool((small == -5.0).all())
    print(json.dumps(dict(math=D.MATH, window=window, refused=refused, err=float(((got - ref).abs() / norm).max()), finite=bool(torch.isfinite(got).all()),
                          shape=list(got.shape))))


if __name__ == "__main__":
    main()
