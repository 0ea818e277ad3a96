"""Planted inputs for the CenterHead post-processing tests (shared by the GPU test and by the CPU computation of the
redraw share).  A discrete decision of the float32 kernel can differ from the float64 yardstick only where a float32
quantity sits on a threshold, so the inputs stay off every threshold BY CONSTRUCTION:

  * scores are planted: background logits below logit(0.05); object cells get scores from a shuffled arithmetic grid in
    (0.1 + 1e-3, 0.99) with spacing >= 1e-5, logits = float32 of the float64 logit (float32 sigmoid error: ~1e-7);
  * geometry is repaired: while the float64 run has a centre within 1e-4 of a range bound, a squared distance within
    1e-4 of a circle radius or a pair IoU within IOU_BAND = 1e-4 of nms_thr, the later box of the pair is redrawn.  The band is
    the one MEASURED for the shared geometry (csrc/al3d_rbox.h) in tests/anchorhead_cases.py: float32 IoU error up to 2.5e-5
    for centres out to +-50 m, as here, times 4.  ``build`` returns the share of redrawn boxes; the tests assert it stays below 1 %.
"""
import numpy as np

import center_fp64 as C

NUSC_TASKS = [1, 2, 2, 1, 2, 2]
F32 = lambda v: float(np.float32(v))      # noqa: E731  constants as the kernel holds them
IOU_BAND = 1e-4                           # 4 x the measured float32 IoU error at range (tests/anchorhead_cases.py)


def layout(task_ncls, vel=True, reg=True, novel_tasks=(), noreg_tasks=()):
    """-> (CH, chan_off rows in detector_ops.CENTER_CHANNELS order: heatmap, reg, height, dim, rot, vel)."""
    rows, o = [], 0
    for t, n in enumerate(task_ncls):
        r = {}
        for name, c in (("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2), ("heatmap", n)):
            if (name == "vel" and (not vel or t in novel_tasks)) or (name == "reg" and (not reg or t in noreg_tasks)):
                r[name] = -1
                continue
            r[name] = o
            o += c
        rows.append([r["heatmap"], r["reg"], r["height"], r["dim"], r["rot"], r["vel"]])
    return o, rows


def params(size, **over):
    p = dict(swapped=True, max_num=500, norm_bbox=True, out_size_factor=8.0, voxel_size=[F32(0.075), F32(0.075)],
             pc_range=[-54.0, -54.0], coder_score_threshold=F32(0.1), post_center_range=[-50.0, -50.0, -5.0, 50.0, 50.0, 3.0],
             nms_type="rotate", nms_scale=[[1.0] * n for n in NUSC_TASKS], min_radius=[4, 12, 10, 1, 0.85, 0.175],
             score_threshold=F32(0.1), nms_thr=F32(0.2), pre_max_size=1000, post_max_size=83,
             post_center_limit_range=[-45.0, -45.0, -4.0, 45.0, 45.0, 2.5], merge=True)
    p.update(over)
    return p


def _draw_geometry(rng, n):
    """reg 2, height 1, log-dim 3, rot 2, vel 2 for n boxes."""
    return np.concatenate([rng.uniform(0.02, 0.98, (n, 2)), rng.uniform(-6.0, 4.0, (n, 1)),
                           np.log(rng.uniform([1.5, 0.6, 1.0], [5.0, 2.2, 2.5], (n, 3))),
                           rng.normal(0, 1, (n, 2)), rng.normal(0, 3, (n, 2))], axis=1).astype(np.float32)


def build(size, B, counts, seed, p, vel=True, reg=True, novel_tasks=(), noreg_tasks=(), task_ncls=NUSC_TASKS):
    """counts[t] = objects per class of task t (a list per class).  -> (hout [B,size,size,CH] f32, chan_off, share of
    redrawn boxes, float64 result of the final inputs)."""
    rng = np.random.default_rng(seed)
    CH, chan = layout(task_ncls, vel, reg, novel_tasks, noreg_tasks)
    hw = size * size
    h = rng.normal(0, 1, (B, hw, CH)).astype(np.float32)
    owners = {}                                          # (b, t) -> cells of the planted objects
    lo = np.log(0.05 / 0.95) - 0.1
    total = 0
    for b in range(B):
        for t, ncls in enumerate(task_ncls):
            heat = chan[t][0]
            h[b, :, heat:heat + ncls] = rng.uniform(lo - 6.0, lo, (hw, ncls))
            n_all = int(sum(counts[t]))
            if n_all == 0:
                owners[(b, t)] = np.zeros(0, np.int64)
                continue
            grid = np.linspace(0.1 + 1e-3, 0.99, n_all + 2)[1:-1]
            assert n_all < 2 or grid[1] - grid[0] >= 1e-5
            rng.shuffle(grid)
            cells = rng.choice(hw, n_all, replace=False)      # one object per cell and task: its geometry is its own
            cls = np.repeat(np.arange(ncls), counts[t])
            h[b, cells, heat + cls] = np.log(grid / (1.0 - grid)).astype(np.float32)
            _write_geometry(h, b, cells, chan[t], _draw_geometry(rng, n_all))
            owners[(b, t)] = cells
            total += n_all
    h = h.reshape(B, size, size, CH)
    redrawn = set()
    for _ in range(20):
        pairs = {}
        ref = C.postprocess(h, task_ncls, chan, pairs=pairs, **p)
        bad = _near_threshold(ref, pairs, p, task_ncls)
        if not bad:
            break
        flat = h.reshape(B, hw, CH)
        for (b, t, cell) in bad:
            _write_geometry(flat, b, np.array([cell]), chan[t], _draw_geometry(rng, 1))
            redrawn.add((b, t, cell))
    else:
        raise AssertionError("the geometry repair did not converge")
    return h, chan, len(redrawn) / max(total, 1), ref


def _write_geometry(h, b, cells, row, geo):
    _, reg, hei, dim, rot, vel = row
    if reg >= 0:
        h[b, cells, reg:reg + 2] = geo[:, 0:2]
    h[b, cells, hei] = geo[:, 2]
    h[b, cells, dim:dim + 3] = geo[:, 3:6]
    h[b, cells, rot:rot + 2] = geo[:, 6:8]
    if vel >= 0:
        h[b, cells, vel:vel + 2] = geo[:, 8:10]


def _near_threshold(ref, pairs, p, task_ncls):
    kinds = [p["nms_type"]] * len(task_ncls) if isinstance(p["nms_type"], str) else p["nms_type"]
    bad = set()
    for b, row in enumerate(ref):
        for t, r in enumerate(row):
            dec = r["decoded"]
            thr = dec["all_scores"] > 0.09                    # the planted objects among the K candidates
            xyz, cells = dec["all_boxes"][thr, :3], dec["all_cells"][thr]
            for rng6 in (p["post_center_range"], p["post_center_limit_range"]):
                near = (np.abs(xyz[:, None, :] - np.asarray(rng6, np.float64).reshape(2, 3)[None]) < 1e-4).any((1, 2))
                bad.update((b, t, int(c)) for c in cells[near])
            surv = dec["cells"]
            if kinds[t] == "rotate":
                surv = surv[dec["scores"] >= p["score_threshold"]][:p["pre_max_size"]] if p["score_threshold"] > 0 else surv
                for i, j, iou in pairs.get((b, t), ()):
                    if abs(iou - p["nms_thr"]) < IOU_BAND:
                        bad.add((b, t, int(surv[j])))
            else:
                for i, j, d2 in pairs.get((b, t), ()):
                    if abs(d2 - p["min_radius"][t]) < 1e-4:
                        bad.add((b, t, int(surv[j])))
    return bad


# name -> (size, B, counts per task and class, build keywords, parameter overrides)
CASES = {
    # nothing above the threshold in task 3; 700 > K cells above it in the single class of task 0; fewer than K elsewhere
    "rotate_128_b3": (128, 3, [[700], [200, 150], [40, 30], [0], [120, 90], [300, 250]], {},
                      dict(nms_scale=[[1.0], [1.0, 1.2], [0.8, 1.0], [1.0], [1.5, 1.0], [2.0, 4.5]])),
    "circle_128_b1": (128, 1, [[300], [100, 80], [60, 0], [0], [250, 260], [400, 200]], {}, dict(nms_type="circle")),
    "mixed_180_b1_novel_noreg": (180, 1, [[600], [150, 150], [30, 20], [50], [0, 0], [350, 300]],
                                 dict(novel_tasks=(1, 4), noreg_tasks=(2, 5)),
                                 dict(nms_type=["rotate", "circle", "rotate", "circle", "rotate", "circle"])),
    "rotate_180_b3_plain": (180, 3, [[90], [60, 50], [20, 10], [30], [0, 40], [200, 100]], dict(vel=False, reg=False), {}),
}


def make(name):
    size, B, counts, bkw, over = CASES[name]
    p = params(size, **over)
    seed = sorted(CASES).index(name) + 7
    h, chan, share, ref = build(size, B, counts, seed, p, **bkw)
    return h, chan, share, ref, p


if __name__ == "__main__":                                   # the redraw shares quoted in tests/test_centerhead_gpu.py
    for name in CASES:
        _, _, share, ref, _ = make(name)
        print(name, f"redrawn share {share:.5f}", "detections", [[len(r["scores"]) for r in row] for row in ref])
