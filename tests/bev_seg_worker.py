"""Child process of tests/test_bev_seg_gpu.py: the BEV segmentation head on the golden input under the AL3D_MATH of the
environment, against the float64 yardstick and the reference golden.  Prints one JSON line: the arithmetic, the largest
error as a fraction of the elementwise bound (tests/test_bev_seg_gpu.py, 'Head'), the error against the golden as a
fraction of its largest magnitude, whether the output is finite, and its shape."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main():
    from test_bev_seg_cpu import golden, scopes
    from test_bev_seg_gpu import golden_head, head_bounds, nhwc
    from al3d import detector_ops as D
    g = golden()
    i_s, o_s = scopes(g["cfg"])
    ref, bound = head_bounds(g["x"], g["sd"], i_s, o_s, 32)
    with torch.no_grad():
        prob = golden_head()(nhwc(g["x"]).to("cuda:0"))
    torch.cuda.synchronize()
    got = prob.cpu().double()
    gold = g["prob"].double()
    print(json.dumps(dict(math=D.MATH, err_over_bound=float(((got - ref["prob"]).abs() / bound).max()),
                          golden=float((got - gold).abs().max() / gold.abs().max()), finite=bool(torch.isfinite(got).all()),
                          shape=list(got.shape))))


if __name__ == "__main__":
    main()
