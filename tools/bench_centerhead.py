"""Times the CenterHead post-processing at B 16 on the 180 x 180 map: the fused device call
(``al3d_center_decode_nms_f32`` through ``detector_ops.center_decode_nms`` + the one read of the counts + the per-sample
merge) against the same post-processing written with torch ops on the same device -- the plain port of
centerpoint.py:637-757 and centerpoint_bbox_coders.py:62-225, kept in this tool and out of the product.

The port follows the reference line by line: per task two ``topk``, the gathers, the elementwise decode, a boolean-mask
index per sample (a host synchronisation each) and the NMS.  ``circle``: the reference's form, a device-to-host copy and
the host loop (``al3d.models.transfusion_head.circle_nms``, the restatement of box3d_nms.py:180-219).  ``rotate``: the
reference calls a CUDA kernel (``nms_gpu``) and copies its mask to the host; there is no torch-op form of it, so the port's
``rotate`` time covers everything EXCEPT the suppression (it keeps the first post_max_size boxes): a lower bound of the
port, against the fused call WITH its suppression.

Each side runs in a child process of its own under its own time limit: warm-up, then rounds of timed calls, host clock
around work that ends in a device synchronise; the median and the spread of the rounds are printed as one JSON line, with
a ``digest`` of the last call's boxes, scores and labels, so that two builds of the library can be compared bit for bit.

  python tools/bench_centerhead.py [--batch 16] [--size 180] [--rounds 7] [--calls 10]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TASKS = [1, 2, 2, 1, 2, 2]
CFG = dict(max_num=500, out_size_factor=8, voxel_size=[0.075, 0.075], pc_range=[-54.0, -54.0], coder_thr=0.1,
           post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], min_radius=[4, 12, 10, 1, 0.85, 0.175], score_threshold=0.1,
           nms_thr=0.2, pre_max_size=1000, post_max_size=83, limit=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0])


def layout():
    rows, o = [], 0
    for n in TASKS:
        r = {}
        for name, c in (("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2), ("heatmap", n)):
            r[name] = o
            o += c
        rows.append(r)
    return o, rows


def make_input(B, size, dev):
    """Head output [B, size, size, CH]: about 1.5 % of the cells of every class above the score threshold."""
    import torch
    CH, rows = layout()
    g = torch.Generator(device=dev).manual_seed(0)
    h = torch.randn(B, size, size, CH, generator=g, device=dev)
    for r, n in zip(rows, TASKS):
        h[..., r["heatmap"]:r["heatmap"] + n] = h[..., r["heatmap"]:r["heatmap"] + n] * 1.5 - 5.5
        h[..., r["dim"]:r["dim"] + 3] = h[..., r["dim"]:r["dim"] + 3] * 0.3 + 0.5
    return h.contiguous(), rows


def fused(h, rows, kind):
    import torch
    from al3d import detector_ops as D
    chan = [[r[k] for k in ("heatmap", "reg", "height", "dim", "rot", "vel")] for r in rows]
    boxes, scores, labels, counts = D.center_decode_nms(
        h, TASKS, chan, swapped=True, max_num=CFG["max_num"], norm_bbox=True, out_size_factor=CFG["out_size_factor"],
        voxel_size=CFG["voxel_size"], pc_range=CFG["pc_range"], coder_score_threshold=CFG["coder_thr"],
        post_center_range=CFG["post_center_range"], nms_type=kind, nms_scale=[[1.0] * n for n in TASKS], min_radius=CFG["min_radius"],
        score_threshold=CFG["score_threshold"], nms_thr=CFG["nms_thr"], pre_max_size=CFG["pre_max_size"],
        post_max_size=CFG["post_max_size"], post_center_limit_range=CFG["limit"], merge=True)
    out = []
    for b, row in enumerate(counts.cpu().tolist()):
        out.append((torch.cat([boxes[b, k, :n] for k, n in enumerate(row)]), torch.cat([scores[b, k, :n] for k, n in enumerate(row)]),
                    torch.cat([labels[b, k, :n] for k, n in enumerate(row)])))
    return out


def torch_port(h, rows, kind):
    """centerpoint.py:637-757 with torch ops.  The map is [B, y, x, C]; the reference's is [B, C, x, y]."""
    import torch
    from al3d.models.transfusion_head import circle_nms
    K = CFG["max_num"]
    nchw = h.permute(0, 3, 2, 1)                                              # [B, C, x, y] view
    rets = []
    for t, (r, ncls) in enumerate(zip(rows, TASKS)):
        m = lambda k, n: nchw[:, r[k]:r[k] + n]                              # noqa: E731
        heat = m("heatmap", ncls).sigmoid()
        dim = torch.exp(m("dim", 3))
        B, cat, height, width = heat.shape
        topk_scores, topk_inds = torch.topk(heat.reshape(B, cat, -1), K)        # coder :79-100
        topk_inds = topk_inds % (height * width)
        topk_xs = (topk_inds.float() / torch.tensor(width, dtype=torch.float)).int().float()
        topk_ys = (topk_inds % width).int().float()
        topk_score, topk_ind = torch.topk(topk_scores.view(B, -1), K)
        clses = (topk_ind / torch.tensor(K, dtype=torch.float)).int()
        inds = topk_inds.view(B, -1).gather(1, topk_ind)
        ys = topk_ys.view(B, -1).gather(1, topk_ind)
        xs = topk_xs.view(B, -1).gather(1, topk_ind)

        def tg(feat):                                                         # _transpose_and_gather_feat
            feat = feat.permute(0, 2, 3, 1).contiguous()
            feat = feat.view(feat.size(0), -1, feat.size(3))
            return feat.gather(1, inds.unsqueeze(2).expand(B, K, feat.size(2)))
        reg = tg(m("reg", 2))
        xs = xs.view(B, K, 1) + reg[:, :, 0:1]
        ys = ys.view(B, K, 1) + reg[:, :, 1:2]
        rot = torch.atan2(tg(m("rot", 2)[:, 0:1]), tg(m("rot", 2)[:, 1:2]))
        hei, dims, vel = tg(m("height", 1)), tg(dim), tg(m("vel", 2))
        xs = xs * CFG["out_size_factor"] * CFG["voxel_size"][0] + CFG["pc_range"][0]
        ys = ys * CFG["out_size_factor"] * CFG["voxel_size"][1] + CFG["pc_range"][1]
        final = torch.cat([xs, ys, hei, dims, rot, vel], dim=2)
        thresh_mask = topk_score > CFG["coder_thr"]
        rng = torch.tensor(CFG["post_center_range"], device=h.device)
        mask = (final[..., :3] >= rng[:3]).all(2) & (final[..., :3] <= rng[3:]).all(2)
        task = []
        for i in range(B):
            cmask = mask[i] & thresh_mask[i]
            boxes3d, scores, labels = final[i, cmask], topk_score[i, cmask], clses[i, cmask]     # boolean-mask index: host sync
            if kind == "circle":
                dets = torch.cat([boxes3d[:, [0, 1]], scores.view(-1, 1)], dim=1)
                keep = torch.tensor(circle_nms(dets.detach().cpu().numpy(), CFG["min_radius"][t], post_max_size=CFG["post_max_size"]),
                                    dtype=torch.long, device=h.device)
            else:                                                             # no torch-op rotated NMS: see the module docstring
                ok = scores >= CFG["score_threshold"]
                boxes3d, scores, labels = boxes3d[ok], scores[ok], labels[ok]
                keep = torch.arange(min(CFG["post_max_size"], scores.shape[0]), device=h.device)
            task.append((boxes3d[keep], scores[keep], labels[keep]))
        rets.append(task)
    out = []
    for i in range(h.shape[0]):
        bboxes = torch.cat([ret[i][0] for ret in rets])
        bboxes[:, 2] = bboxes[:, 2] - bboxes[:, 5] * 0.5
        flag, labels = 0, []
        for j, n in enumerate(TASKS):
            labels.append(rets[j][i][2].int() + flag)
            flag += n
        out.append((bboxes, torch.cat([ret[i][1] for ret in rets]), torch.cat(labels)))
    return out


def child(side, kind, B, size, rounds, calls):
    import torch
    dev = torch.device("cuda:0")
    h, rows = make_input(B, size, dev)
    fn = fused if side == "fused" else torch_port
    with torch.no_grad():
        for _ in range(3):
            out = fn(h, rows, kind)
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            for _ in range(calls):
                out = fn(h, rows, kind)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / calls)
    h = hashlib.sha256()
    for o in out:
        for t in o:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    print(json.dumps(dict(side=side, nms=kind, batch=B, size=size, digest=h.hexdigest()[:16], ms_per_batch=round(statistics.median(ms), 3),
                          ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), rounds=rounds, calls_per_round=calls,
                          detections_per_sample=round(sum(len(o[1]) for o in out) / B, 1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=180)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.batch, a.size, a.rounds, a.calls)
    res = {}
    for kind in ("rotate", "circle"):
        for side in ("fused", "torch", "fused", "torch"):                     # alternating: the spread between repeats shows
            cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--size", str(a.size), "--rounds", str(a.rounds),
                   "--calls", str(a.calls), "--child", side, kind]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:
                print(r.stderr[-2000:], file=sys.stderr)
                return 1                                                      # a failed side ends the tool: nothing more is started
            line = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(line), flush=True)
            res.setdefault((kind, side), []).append(line["ms_per_batch"])
    for kind in ("rotate", "circle"):
        f, t = min(res[(kind, "fused")]), min(res[(kind, "torch")])
        print(json.dumps(dict(nms=kind, fused_ms=f, torch_port_ms=t, ratio=round(t / f, 2),
                              note="torch port WITHOUT the suppression" if kind == "rotate" else "torch port with the host circle_nms")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
