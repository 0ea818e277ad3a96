"""Shared pieces of the tests of the anchor head's other box codes and its direction classifier
(``al3d_head_decode_nms_codes``, ``al3d_box_decode_codes_f32``, ``MultiGroupHead`` with ``loss_aux``):

* the goldens of tools/gen_golden_anchor_head_codes.py (tests/golden/head_predict_codes.npz: the reference's own
  ``MultiGroupHead.predict`` with ``use_direction_classifier``) as cases, and the fused head record the library reads;
* a float64 numpy restatement of decode + selection + rotated NMS + direction fix-up + range mask (selection and NMS are
  tests/head_fp64.py's), held to the goldens by tests/test_anchorhead_codes_cpu.py;
* the planted exact edges of the fix-up, whose expectation is torch's own float32 arithmetic on the CPU;
* the library runners.

Tolerances are those tests/test_head_predict_golden.py uses for this kernel: labels and order equal, scores 1.2e-7 relative,
box columns 2e-6, angles 1e-5 modulo 2 pi.
"""
import ctypes
import os

import numpy as np

import head_fp64 as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_predict_codes.npz")
F32 = lambda v: float(np.float32(v))      # noqa: E731
PI32 = np.float32(np.pi)
SENTINEL = -7777.0
_z = None


def gold():
    global _z
    if _z is None:
        _z = dict(np.load(GOLD))
    return _z


def case_names():
    return [str(n) for n in gold()["cases"]]


def load(name):
    """-> dict(n_dim, vec, with_dir, offset, seed, B, H, W, nc, na, box/cls/dirs/anchors per task, ref per sample, params)."""
    z = gold()
    n_dim, vec, with_dir, offset, seed = z[f"{name}.cfg"]
    B, Hh, W = (int(v) for v in z["shape"])
    nc = [int(v) for v in z["num_classes"]]
    thr, iou, pre, post = z["params"]
    nt = len(nc)
    return dict(name=name, n_dim=int(n_dim), vec=int(vec), with_dir=bool(with_dir), offset=float(offset), seed=int(seed),
                B=B, H=Hh, W=W, nc=nc, na=[2 * c for c in nc],
                box=[z[f"{name}.box{t}"] for t in range(nt)], cls=[z[f"{name}.cls{t}"] for t in range(nt)],
                dirs=[z[f"{name}.dir{t}"] if with_dir else None for t in range(nt)],
                anchors=[z[f"{name}.anchors{t}"] for t in range(nt)],
                ref=[dict(boxes=z[f"{name}.out{b}.boxes"], scores=z[f"{name}.out{b}.scores"], labels=z[f"{name}.out{b}.labels"])
                     for b in range(B)],
                params=dict(score_thresh=float(thr), iou_thresh=float(iou), pre_max=int(pre), post_max=int(post),
                            rng=[float(v) for v in z["range"]]))


def fused(case, lead=0, gap=0, tail=0, with_dir=None, fill=0.25):
    """The head's fused record [B, HW, CH] in the order [lead | all box | all class | gap | all dir | tail] with ``fill`` in the
    padding -> (hout, box_off, cls_off, dir_off).  ``with_dir=False`` leaves the classifier out (dir_off all -1)."""
    with_dir = case["with_dir"] if with_dir is None else with_dir
    B, HW = case["B"], case["H"] * case["W"]
    nt = len(case["nc"])
    parts, offs, pos = [], {"box": [], "cls": [], "dir": []}, 0

    def add(kind, arr):
        nonlocal pos
        a = arr.reshape(B, HW, -1)
        if kind:
            offs[kind].append(pos)
        parts.append(a)
        pos += a.shape[2]
    pad = lambda w: np.full((B, HW, w), fill, np.float32)      # noqa: E731
    if lead:
        add(None, pad(lead))
    for t in range(nt):
        add("box", case["box"][t])
    for t in range(nt):
        add("cls", case["cls"][t])
    if gap:
        add(None, pad(gap))
    if with_dir:
        for t in range(nt):
            add("dir", case["dirs"][t])
    if tail:
        add(None, pad(tail))
    hout = np.ascontiguousarray(np.concatenate(parts, axis=2), dtype=np.float32)
    return hout, offs["box"], offs["cls"], offs["dir"] if with_dir else [-1] * nt


def odd_layout(case):
    """The record with one padding channel in front and one before the direction window, and an odd CH: no window 16-byte
    aligned, the score pre-pass on its scalar path."""
    ch = fused(case, lead=1, gap=1)[0].shape[2]
    return fused(case, lead=1, gap=1, tail=0 if ch % 2 else 1)


# ---------------------------------------------------------------------------------------------- numpy restatement
def decode(enc, anchors, n_dim, vec):
    """second_box_decode (box_torch_ops.py:80-148; smooth_dim and norm_velo never reach it, box_coders.py:106-109) in float64:
    enc [n, n_dim + vec], anchors [n, n_dim] -> [n, n_dim]."""
    t, a = np.asarray(enc, np.float64).reshape(-1, n_dim + vec), np.asarray(anchors, np.float64).reshape(-1, n_dim)
    diag = np.sqrt(a[:, 4] ** 2 + a[:, 3] ** 2)
    with np.errstate(over="ignore", invalid="ignore"):
        cols = [t[:, 0] * diag + a[:, 0], t[:, 1] * diag + a[:, 1], t[:, 2] * a[:, 5] + a[:, 2],
                np.exp(t[:, 3]) * a[:, 3], np.exp(t[:, 4]) * a[:, 4], np.exp(t[:, 5]) * a[:, 5]]
        if n_dim == 9:
            cols += [t[:, 6] + a[:, 6], t[:, 7] + a[:, 7]]
        ra = a[:, n_dim - 1]
        cols.append(np.arctan2(t[:, n_dim] + np.sin(ra), t[:, n_dim - 1] + np.cos(ra)) if vec else t[:, n_dim - 1] + ra)
    return np.stack(cols, axis=1)


def dir_labels(logits):
    """torch.max(dir_preds, dim=-1)[1] on [n, 2]: 1 iff l1 > l0, or l1 is NaN and l0 is not."""
    l0, l1 = logits[:, 0], logits[:, 1]
    with np.errstate(invalid="ignore"):
        return (l1 > l0) | (np.isnan(l1) & ~np.isnan(l0))


def fixup(r, labels, offset):
    """mg_head.py:1042-1051: r += pi (float32 np.pi) where ((r - offset) > 0) xor label."""
    with np.errstate(invalid="ignore"):
        opp = ((r - np.float64(np.float32(offset))) > 0) ^ labels
    return r + np.where(opp, np.float64(PI32), 0.0)


def task_predict(hout, anchors, na, nc, box_off, cls_off, dir_off, n_dim, vec, offset, p):
    """One (sample, task): hout [HW, CH] -> (boxes [k, n_dim], scores, labels) in output order."""
    hw = hout.shape[0]
    code = n_dim + vec
    order, score, label = H.select(hout[:, cls_off:cls_off + na * nc].reshape(hw * na, nc), F32(p["score_thresh"]), p["pre_max"])
    boxes = decode(hout[:, box_off:box_off + na * code].reshape(hw * na, code)[order], np.asarray(anchors)[order], n_dim, vec)
    keep = np.asarray(H.rotate_nms(boxes[:, [0, 1, 3, 4, n_dim - 1]], F32(p["iou_thresh"]), p["post_max"]), np.int64)
    b = boxes[keep].copy()
    if dir_off >= 0:                                                   # after the NMS, on the survivors only
        lg = hout[:, dir_off:dir_off + na * 2].reshape(hw * na, 2)[order[keep]].astype(np.float64)
        b[:, -1] = fixup(b[:, -1], dir_labels(lg), offset)
    r = np.asarray(p["rng"], np.float64)
    ok = (b[:, :3] >= r[:3]).all(1) & (b[:, :3] <= r[3:]).all(1)
    return b[ok], score[keep][ok], label[keep][ok]


def predict(case, layout=None):
    """The restatement on a golden case -> [dict(boxes, scores, labels) per sample], tasks merged with the label offsets."""
    hout, box_off, cls_off, dir_off = layout if layout is not None else fused(case)
    loff = np.concatenate([[0], np.cumsum(case["nc"])])
    out = []
    for b in range(case["B"]):
        bb, ss, ll = [], [], []
        for t, nc in enumerate(case["nc"]):
            bx, sc, lb = task_predict(hout[b], case["anchors"][t], case["na"][t], nc, box_off[t], cls_off[t], dir_off[t],
                                      case["n_dim"], case["vec"], case["offset"], case["params"])
            bb.append(bx); ss.append(sc); ll.append(lb + loff[t])
        out.append(dict(boxes=np.concatenate(bb), scores=np.concatenate(ss), labels=np.concatenate(ll)))
    return out


def assert_close(got, ref, where=""):
    """got / ref: dict(boxes [k, D], scores, labels) -- the tolerances of the module docstring."""
    assert np.asarray(got["labels"]).tolist() == np.asarray(ref["labels"]).tolist(), (where, got["labels"], ref["labels"])
    gs, rs = np.asarray(got["scores"], np.float64), np.asarray(ref["scores"], np.float64)
    assert np.all(np.abs(gs - rs) <= 1.2e-7 * np.maximum(np.abs(rs), 1e-3)), (where, np.abs(gs - rs).max())
    gb, rb = np.asarray(got["boxes"], np.float64), np.asarray(ref["boxes"], np.float64)
    assert gb.shape == rb.shape, (where, gb.shape, rb.shape)
    np.testing.assert_allclose(gb[:, :-1], rb[:, :-1], rtol=2e-6, atol=2e-6, err_msg=where)
    d = np.abs(gb[:, -1] - rb[:, -1])
    assert len(d) == 0 or np.minimum(d, np.abs(2 * np.pi - d)).max() < 1e-5, (where, d.max())


def bands(case):
    """The generator's edge bands recomputed from the committed arrays (float64 here, the reference's float32 there) ->
    dict of the smallest distances to each edge over the case, and whether both cuts bite in every non-empty (sample, task)."""
    import anchorhead_cases as AC
    p = case["params"]
    thr, iou = np.float64(np.float32(p["score_thresh"])), np.float64(np.float32(p["iou_thresh"]))
    out = dict(score_gap=np.inf, score_thr=np.inf, angle=np.inf, dir=np.inf, iou=np.inf, cuts=True, empty=[])
    for t, nc in enumerate(case["nc"]):
        na, code = case["na"][t], case["n_dim"] + case["vec"]
        for b in range(case["B"]):
            s = H.sigmoid(case["cls"][t][b].reshape(-1, nc))
            out["score_thr"] = min(out["score_thr"], np.abs(s - thr).min())
            top = np.sort(s.max(1)[s.max(1) >= thr])
            if len(top) > 1:
                out["score_gap"] = min(out["score_gap"], np.diff(top).min())
            dec = decode(case["box"][t][b].reshape(-1, code), case["anchors"][t], case["n_dim"], case["vec"])
            out["angle"] = min(out["angle"], np.abs(dec[:, -1] - np.float64(np.float32(case["offset"]))).min())
            if case["with_dir"]:
                d = case["dirs"][t][b].reshape(-1, 2).astype(np.float64)
                out["dir"] = min(out["dir"], np.abs(d[:, 1] - d[:, 0]).min())
            if len(top) == 0:
                out["empty"].append((b, t))
                continue
            order, _, _ = H.select(case["cls"][t][b].reshape(-1, nc), thr, p["pre_max"])
            pairs = []
            keep = H.rotate_nms(dec[order][:, [0, 1, 3, 4, -1]], iou, p["post_max"], pairs)
            for _, _, q in pairs:
                out["iou"] = min(out["iou"], abs(q["iou"] - iou))
            out["cuts"] &= len(top) > p["pre_max"] and len(keep) == p["post_max"]
    out["iou_delta"] = AC.DELTA["origin"]
    return out


# ---------------------------------------------------------------------------------------------- planted exact edges
EDGE_RANGE = [-100.0, -100.0, -3.0, 100.0, 100.0, 1.5]
EDGE_NAMES = ["r==off label1", "r==off label0", "equal logits r>off", "equal logits r<off", "[nan,x]", "[x,nan]", "[nan,nan]",
              "r=off+ulp label0", "r=off+ulp label1", "r=off-ulp label0", "r=off-ulp label1", "z==range[5] flipped",
              "z>range[5] flipped", "z==range[5] kept angle", "-inf logit"]


def edge_case(n_dim, offset):
    """Scalar-code plants, one per location of a 4 x 4 map (anchor 0 of the location; 10 m apart, 1 x 1 m: the NMS never
    acts), rt = 0 so that the decoded angle IS the anchor's (0 + ra is exact).  Scores descend with the plant index.
    -> (case dict for ``run_codes``, plants = list of (name, anchor index, ra float32, logits float32 [2], z))."""
    off32 = np.float32(offset)
    up, dn = np.nextafter(off32, np.float32(np.inf)), np.nextafter(off32, np.float32(-np.inf))
    nan = np.float32(np.nan)
    zt = np.float32(EDGE_RANGE[5])
    spec = [(off32, (0.3, 0.9), 0.0), (off32, (0.9, 0.3), 0.0), (off32 + np.float32(0.5), (0.5, 0.5), 0.0),
            (off32 - np.float32(0.5), (0.5, 0.5), 0.0), (off32 + np.float32(0.5), (nan, 0.1), 0.0),
            (off32 + np.float32(0.5), (0.1, nan), 0.0), (off32 - np.float32(0.5), (nan, nan), 0.0),
            (up, (0.9, 0.3), 0.0), (up, (0.3, 0.9), 0.0), (dn, (0.9, 0.3), 0.0), (dn, (0.3, 0.9), 0.0),
            (off32 + np.float32(0.5), (0.9, 0.3), zt), (off32 + np.float32(0.5), (0.9, 0.3), np.nextafter(zt, np.float32(np.inf))),
            (off32 + np.float32(0.5), (0.3, 0.9), zt), (off32 - np.float32(0.5), (-np.inf, 0.0), 0.0)]
    assert len(spec) == len(EDGE_NAMES)
    Hh = W = 4
    na, nc = 2, 1
    HW = Hh * W
    anchors = np.zeros((HW * na, n_dim), np.float32)
    for loc in range(HW):
        for j in range(na):
            a = loc * na + j
            anchors[a, :6] = [10.0 * (loc % W) - 15.0, 10.0 * (loc // W) - 15.0, 0.0, 1.0, 1.0, 1.0]
            anchors[a, n_dim - 1] = 0.3 * j
    CH = 1 + na * n_dim + na * nc + 1 + na * 2            # [pad | box | cls | pad | dir]: CH even or odd, windows unaligned
    box_off, cls_off, dir_off = 1, 1 + na * n_dim, 1 + na * n_dim + na * nc + 1
    hout = np.zeros((1, HW, CH), np.float32)
    hout[..., cls_off:cls_off + na * nc] = -20.0
    hout[..., dir_off:dir_off + na * 2] = 7.0             # the sleeping anchors' logits are never read
    plants = []
    for k, (ra, lg, z) in enumerate(spec):
        loc, a = k, k * na
        anchors[a, 2] = z
        anchors[a, n_dim - 1] = ra
        hout[0, loc, cls_off] = np.float32(3.0 - 0.1 * k)
        hout[0, loc, dir_off:dir_off + 2] = lg
        plants.append((EDGE_NAMES[k], a, np.float32(ra), np.array(lg, np.float32), np.float32(z)))
    case = dict(n_dim=n_dim, vec=0, offset=float(offset), B=1, H=Hh, W=W, nc=[nc], na=[na], anchors=[anchors],
                params=dict(score_thresh=0.1, iou_thresh=0.2, pre_max=64, post_max=16, rng=EDGE_RANGE))
    return case, (hout, [box_off], [cls_off], [dir_off]), plants


def edge_expected(plants, offset, n_dim):
    """torch on the CPU, float32, the reference's own lines (mg_head.py:842,1044-1051,1056-1057) on the planted boxes."""
    import torch
    r = torch.tensor([float(p[2]) for p in plants], dtype=torch.float32)
    box = torch.zeros((len(plants), n_dim), dtype=torch.float32)
    box[:, 2] = torch.tensor([float(p[4]) for p in plants], dtype=torch.float32)
    box[:, -1] = r
    dir_preds = torch.from_numpy(np.stack([p[3] for p in plants]))
    dir_labels_ = torch.max(dir_preds, dim=-1)[1]
    opp = ((box[..., -1] - offset) > 0) ^ dir_labels_.bool()
    box[..., -1] += torch.where(opp, torch.tensor(np.pi).type_as(box), torch.tensor(0.0).type_as(box))
    rng = torch.tensor(EDGE_RANGE, dtype=torch.float32)
    mask = (box[:, 2] >= rng[2]) & (box[:, 2] <= rng[5])
    return box[:, -1].numpy(), opp.numpy(), mask.numpy()


# ---------------------------------------------------------------------------------------------- library runners
def _args(case, layout, dev):
    import torch
    hout_np, box_off, cls_off, dir_off = layout
    p = case["params"]
    hout = torch.from_numpy(hout_np).to(dev).contiguous()
    B, HW, CH = hout.shape
    nt, post = len(case["na"]), p["post_max"]
    a_dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in case["anchors"]]
    IntA = ctypes.c_int * nt
    loff = np.concatenate([[0], np.cumsum(case["nc"])])[:nt]
    vp = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
    head = (vp(hout), B, HW, CH, nt, (ctypes.c_void_p * nt)(*[a.data_ptr() for a in a_dev]),
            IntA(*[a.shape[0] for a in a_dev]), IntA(*case["na"]), IntA(*case["nc"]), IntA(*box_off), IntA(*cls_off),
            IntA(*[int(v) for v in loff]), float(p["score_thresh"]), float(p["iou_thresh"]), int(p["pre_max"]), post,
            (ctypes.c_float * 6)(*[float(v) for v in p["rng"]]))
    return head, (hout, a_dev), IntA(*dir_off), (B, nt, post)


def run_codes(case, layout, old_entry=False):
    """``al3d_head_decode_nms_codes`` (or, ``old_entry``, ``al3d_head_decode_nms``) -> (boxes [B,nt,post,n_dim], scores, labels,
    counts) as numpy arrays, the outputs pre-filled with SENTINEL."""
    import torch
    from al3d import lib
    dev = torch.device("cuda:0")
    head, hold, dir_off, (B, nt, post) = _args(case, layout, dev)
    boxes = torch.full((B, nt, post, case["n_dim"]), SENTINEL, dtype=torch.float32, device=dev)
    scores = torch.full((B, nt, post), SENTINEL, dtype=torch.float32, device=dev)
    labels = torch.full((B, nt, post), int(SENTINEL), dtype=torch.int32, device=dev)
    counts = torch.full((B, nt), int(SENTINEL), dtype=torch.int32, device=dev)
    ws = torch.empty(lib.load().al3d_head_decode_nms_workspace_bytes(B, nt, head[6]), dtype=torch.uint8, device=dev)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
    outs = (vp(boxes), vp(scores), vp(labels), vp(counts), vp(ws), torch.cuda.current_stream(dev).cuda_stream)
    if old_entry:
        lib.call("al3d_head_decode_nms", *head, *outs)
    else:
        lib.call("al3d_head_decode_nms_codes", *head, case["n_dim"], case["vec"], dir_off, float(case["offset"]), *outs)
    torch.cuda.synchronize(dev)
    del hold
    return boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy()


def merged(got, b, tasks=None):
    """Sample b of the raw buffers -> dict(boxes, scores, labels) over the tasks in order; rows past counts must be untouched."""
    boxes, scores, labels, counts = got
    bb, ss, ll = [], [], []
    for t in (range(boxes.shape[1]) if tasks is None else tasks):
        k = int(counts[b, t])
        assert 0 <= k <= boxes.shape[2]
        assert np.all(boxes[b, t, k:] == SENTINEL) and np.all(scores[b, t, k:] == SENTINEL) and \
            np.all(labels[b, t, k:] == int(SENTINEL)), f"sample {b} task {t}: rows past counts were written"
        bb.append(boxes[b, t, :k]); ss.append(scores[b, t, :k]); ll.append(labels[b, t, :k])
    return dict(boxes=np.concatenate(bb), scores=np.concatenate(ss), labels=np.concatenate(ll))


def refusals():
    """Argument sets ``al3d_head_decode_nms_codes`` must refuse with AL3D_EINVAL before any launch (no GPU is touched: the
    pointers are never dereferenced) -> list of (name, rc, message)."""
    from al3d import lib
    so = lib.load()
    fake = ctypes.c_void_p(4096)
    IntA = ctypes.c_int * 2
    HW, na, nc = 4, [2, 4], [1, 2]

    def call(n_dim=7, vec=0, CH=64, box_off=(0, 14), cls_off=(42, 44), dir_off=(52, 56)):
        rc = so.al3d_head_decode_nms_codes(
            fake, 1, HW, CH, 2, (ctypes.c_void_p * 2)(4096, 4096), IntA(HW * na[0], HW * na[1]), IntA(*na), IntA(*nc),
            IntA(*box_off), IntA(*cls_off), IntA(0, 1), 0.1, 0.2, 64, 16, (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1),
            n_dim, vec, IntA(*dir_off), 0.0, fake, fake, fake, fake, fake, None)
        return rc, so.al3d_last_error().decode()
    # layout: box 0 [0,14), box 1 [14,42), cls 0 [42,44), cls 1 [44,52), dir 0 [52,56), dir 1 [56,64)
    return [("n_dim 8", *call(n_dim=8)), ("n_dim 10", *call(n_dim=10)),
            ("dir in box window", *call(dir_off=(12, 56))), ("dir in class window", *call(dir_off=(52, 50))),
            ("dir straddles class start", *call(dir_off=(41, 56))),
            ("dir past CH", *call(dir_off=(52, 57))), ("mixed -1 first", *call(dir_off=(-1, 56))),
            ("mixed -1 second", *call(dir_off=(52, -1)))]
