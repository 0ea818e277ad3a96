"""Dev tool: time the anchor head's decode + NMS launches (score pre-pass + one workgroup per (sample, task)) on seeded head
outputs, straight through the C-ABI.  Four legs, each ``--repeats`` times ``--iters`` back-to-back calls between two events:

  old     al3d_head_decode_nms on the CBGS shape bench.py sweeps (batch 128, 128 x 128 map, six tasks, CH 236, pre 1000 / post 83)
  vec     al3d_head_decode_nms_codes on the same inputs: 10-wide vector code, no classifier (the same kernel instantiation)
  scalar  al3d_head_decode_nms_codes with scalar 9-dim codes plus the direction classifier on the PointPillars map (128 x 128,
          six tasks, CH 20*9 + 36 + 40 = 256)
  tf      al3d_tf_proposals_f32, the TransFusion query initialisation, on the BEVFusion shape (``--tf-batch`` samples, 180 x 180
          map, 10 classes, 200 proposals, hidden 128)

``--lib PATH`` times another build of the library (a parent commit's, which lacks the new entry: its ``vec`` / ``scalar`` legs
print null), so ``old`` can be compared across commits with the same tool and inputs.  Every leg carries a ``digest`` of its
outputs (the valid rows only), so two builds can be compared bit for bit as well.  Prints one JSON line."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from al3d import lib  # noqa: E402

NUM_CLASSES = [1, 2, 2, 1, 2, 2]


def inputs(B, HW, n_dim, vec, with_dir, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    na = [2 * c for c in NUM_CLASSES]
    code = n_dim + vec
    widths = [a * code for a in na] + [a * c for a, c in zip(na, NUM_CLASSES)] + ([a * 2 for a in na] if with_dir else [])
    offs = np.concatenate([[0], np.cumsum(widths)]).astype(int).tolist()
    nt = len(na)
    CH = offs[-1]
    # one frame's record, repeated with a per-frame shift of the class logits: a few percent of the anchors pass 0.1
    hout = torch.empty((B, HW, CH), dtype=torch.float32)
    hout[:, :, :offs[nt]] = torch.randn((B, HW, offs[nt]), generator=g) * 0.3
    hout[:, :, offs[nt]:offs[2 * nt]] = torch.randn((B, HW, offs[2 * nt] - offs[nt]), generator=g) * 1.5 - 3.5
    if with_dir:
        hout[:, :, offs[2 * nt]:] = torch.randn((B, HW, CH - offs[2 * nt]), generator=g)
    side = int(round(HW ** 0.5))
    anchors = []
    for t, a in enumerate(na):
        an = torch.zeros((HW * a, n_dim), dtype=torch.float32)
        loc = torch.arange(HW).repeat_interleave(a)
        an[:, 0] = (loc % side).float() * (102.4 / side) - 51.2
        an[:, 1] = (loc // side).float() * (102.4 / side) - 51.2
        an[:, 2] = -1.0
        an[:, 3:6] = torch.tensor([[1.97, 4.63, 1.74], [2.51, 6.93, 2.84], [2.94, 10.5, 3.47], [2.53, 0.5, 0.98],
                                   [0.77, 2.11, 1.47], [0.67, 0.73, 1.77]][t])
        an[:, n_dim - 1] = (torch.arange(HW * a) % 2).float() * 1.57
        anchors.append(an.to(dev))
    return dict(hout=hout.to(dev), anchors=anchors, na=na, B=B, HW=HW, CH=CH, box_off=offs[:nt], cls_off=offs[nt:2 * nt],
                dir_off=offs[2 * nt:3 * nt] if with_dir else [-1] * nt, n_dim=n_dim, vec=vec)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def timed(once, iters, repeats, dev):
    once()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            once()
        e1.record()
        torch.cuda.synchronize(dev)
        ms.append(e0.elapsed_time(e1) / iters)
    return dict(ms=[round(v, 4) for v in ms], min=round(min(ms), 4), max=round(max(ms), 4), median=round(float(np.median(ms)), 4))


def leg(so, x, new_entry, iters, repeats, dev, pre=1000, post=83):
    nt = len(x["na"])
    IntA = ctypes.c_int * nt
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    B = x["B"]
    boxes = torch.empty((B, nt, post, x["n_dim"]), dtype=torch.float32, device=dev)
    scores = torch.empty((B, nt, post), dtype=torch.float32, device=dev)
    labels = torch.empty((B, nt, post), dtype=torch.int32, device=dev)
    counts = torch.empty((B, nt), dtype=torch.int32, device=dev)
    task_a = IntA(*[a.shape[0] for a in x["anchors"]])
    ws = torch.empty(so.al3d_head_decode_nms_workspace_bytes(B, nt, task_a), dtype=torch.uint8, device=dev)
    label_off = np.concatenate([[0], np.cumsum(NUM_CLASSES)])[:nt].astype(int).tolist()
    stream = torch.cuda.current_stream(dev).cuda_stream
    head = (vp(x["hout"]), B, x["HW"], x["CH"], nt, (ctypes.c_void_p * nt)(*[a.data_ptr() for a in x["anchors"]]), task_a,
            IntA(*x["na"]), IntA(*NUM_CLASSES), IntA(*x["box_off"]), IntA(*x["cls_off"]), IntA(*label_off), 0.1, 0.2, pre, post,
            (ctypes.c_float * 6)(-61.2, -61.2, -10.0, 61.2, 61.2, 10.0))
    outs = (vp(boxes), vp(scores), vp(labels), vp(counts), vp(ws), stream)

    def once():
        if new_entry:
            rc = so.al3d_head_decode_nms_codes(*head, x["n_dim"], x["vec"], IntA(*x["dir_off"]), 0.0, *outs)
        else:
            rc = so.al3d_head_decode_nms(*head, *outs)
        if rc != 0:
            raise RuntimeError(so.al3d_last_error().decode())
    out = timed(once, iters, repeats, dev)
    valid = torch.arange(post, device=dev)[None, None, :] < counts[:, :, None]
    return dict(out, detections=int(counts.sum().item()), digest=digest(boxes[valid], scores[valid], labels[valid], counts))


def tf_leg(so, B, iters, repeats, dev, side=180, C=10, P=200, hidden=128, seed=2):
    g = torch.Generator(device="cpu").manual_seed(seed)
    HW = side * side
    heat = (torch.randn((B, side, side, C), generator=g) * 1.5 - 3.5).to(dev)
    tokens = torch.randn((B, HW, hidden), generator=g).to(dev)
    bev_pos = torch.randn((HW, 2), generator=g).to(dev)
    cols, bias = torch.randn((C, hidden), generator=g).to(dev), torch.randn((hidden,), generator=g).to(dev)
    top_class = torch.empty((B, P), dtype=torch.int64, device=dev)
    top_cell = torch.empty((B, P), dtype=torch.int64, device=dev)
    qscore = torch.empty((B, C, P), dtype=torch.float32, device=dev)
    qfeat = torch.empty((B, P, hidden), dtype=torch.float32, device=dev)
    qpos = torch.empty((B, P, 2), dtype=torch.float32, device=dev)
    ws = torch.empty(so.al3d_tf_proposals_workspace_bytes(B, side, side, C), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def once():
        rc = so.al3d_tf_proposals_f32(vp(heat), B, side, side, C, 3, (1 << 8) | (1 << 9), P, vp(tokens), hidden, vp(bev_pos), vp(cols),
                                      vp(bias), vp(ws), vp(top_class), vp(top_cell), vp(qscore), vp(qfeat), vp(qpos), stream)
        if rc != 0:
            raise RuntimeError(so.al3d_last_error().decode())
    out = timed(once, iters, repeats, dev)
    return dict(out, batch=B, digest=digest(top_class, top_cell, qscore, qfeat, qpos))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=lib.LIB_PATH)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tf-batch", type=int, default=4)
    args = ap.parse_args()
    so = ctypes.CDLL(args.lib)
    so.al3d_last_error.restype = ctypes.c_char_p
    for name in ("al3d_head_decode_nms", "al3d_head_decode_nms_codes", "al3d_head_decode_nms_workspace_bytes", "al3d_tf_proposals_f32",
                 "al3d_tf_proposals_workspace_bytes"):
        if hasattr(so, name):
            getattr(so, name).restype, getattr(so, name).argtypes = lib.SIGNATURES[name]
    has_new = hasattr(so, "al3d_head_decode_nms_codes")
    dev = torch.device("cuda:0")
    cbgs = inputs(args.batch, 128 * 128, 9, 1, False, dev)
    out = {"lib": os.path.relpath(args.lib, ROOT), "batch": args.batch, "iters": args.iters, "unit": "ms per call",
           "old": leg(so, cbgs, False, args.iters, args.repeats, dev), "vec": None, "scalar": None}
    if has_new:
        out["vec"] = leg(so, cbgs, True, args.iters, args.repeats, dev)
        del cbgs
        out["scalar"] = leg(so, inputs(args.batch, 128 * 128, 9, 0, True, dev, seed=1), True, args.iters, args.repeats, dev)
    out["tf"] = tf_leg(so, args.tf_batch, args.iters, args.repeats, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
