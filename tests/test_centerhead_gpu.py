"""GPU suite of the CenterPoint head: ``al3d_center_decode_nms_f32`` against the float64 restatement
(tests/center_fp64.py), ``al3d_conv3x3_grouped_nhwc_f32`` against a float64 grouped convolution, and the whole head
against an independent NCHW torch evaluation of the same seeded parameters.

Post-processing cases (tests/centerhead_cases.py): maps 128 x 128 and 180 x 180, B 1 and 3, the nuScenes task list,
K 500, both NMS kinds, a per-task ``nms_type`` list, ``nms_scale`` != 1, tasks without ``vel`` / ``reg``, a task with
nothing above the threshold, one with 700 > K cells above it in a single class, the others with fewer than K.  The
inputs stay off every threshold by construction (planted scores, repaired geometry); the share of redrawn boxes,
computed on the CPU with center_fp64 alone (``python tests/centerhead_cases.py``), is 0.00035 for ``rotate_128_b3`` (2 of
5,640 boxes) and 0 for the other three cases; asserted below 1 % here.

Bounds against float64 (not measured: derived).  u = 2^-24.  sigmoid, exp and atan2 are the only inexact library steps
(<= 2 ulp each in the device library), every other step is one float32 rounding:
  * score: expf (2 ulp) + add + divide: relative 4u of a value < 1                         -> 4u  = 2.4e-7 absolute
  * x, y: (cell + reg) * 8 * vs + pc: four roundings of values below 128 in magnitude    -> 4 * u * 128 = 3.1e-5
    (the geometry constants are handed to both sides as the same float32 values)
  * dim: expf: 2 ulp + the rounding of the store                                          -> 4u relative
  * rot: atan2f: 2 ulp of a value <= pi (ulp 2^-22), + rounding                             -> 3 * 2^-22 = 7.2e-7
  * z = height - dim2 / 2: height is exact, dim2 carries 4u relative, one rounding of |z| < 16 -> 2u * dim2 + u * 16
  * vel: copied                                                                           -> 0
"""
import numpy as np
import pytest
import torch

import center_fp64 as C
import centerhead_cases as cases

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _run_kernel(h, chan, p, task_ncls=cases.NUSC_TASKS):
    from al3d import detector_ops as D
    out = D.center_decode_nms(torch.from_numpy(h).cuda(), task_ncls, chan, **p)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _compare(got, ref, name):
    boxes, scores, labels, counts = got
    for b, row in enumerate(ref):
        for t, r in enumerate(row):
            n = len(r["scores"])
            print(f"{name} sample {b} task {t}: float64 keeps {n}, device keeps {int(counts[b, t])}")
            assert int(counts[b, t]) == n, (name, b, t)
            gb, gs, gl = boxes[b, t, :n].astype(np.float64), scores[b, t, :n].astype(np.float64), labels[b, t, :n]
            assert np.array_equal(gl, r["labels"]), (name, b, t, "labels / order")
            assert np.all(np.abs(gs - r["scores"]) <= 4 * U), (name, b, t, "scores / order")
            rb = r["boxes"]
            err = np.abs(gb - rb)
            if n:
                print("   max errors x,y", err[:, :2].max(), "z", err[:, 2].max(), "dim rel", (err[:, 3:6] / rb[:, 3:6]).max(),
                      "rot", err[:, 6].max(), "vel", err[:, 7:].max())
            assert np.all(err[:, :2] <= 4 * U * 128)
            assert np.all(err[:, 3:6] <= 4 * U * rb[:, 3:6])
            assert np.all(err[:, 2] <= 2 * U * rb[:, 5] + U * 16)
            assert np.all(err[:, 6] <= 3 * 2.0 ** -22)
            assert np.all(err[:, 7:] == 0)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_decode_nms_matches_float64(name):
    h, chan, share, ref, p = cases.make(name)
    print(f"{name}: redrawn share {share:.5f}")
    assert share < 0.01
    got = _run_kernel(h, chan, p)
    _compare(got, ref, name)
    again = _run_kernel(h, chan, p)
    n = got[3]
    for b in range(n.shape[0]):
        for t in range(n.shape[1]):
            for a, c in zip(got[:3], again[:3]):
                assert np.array_equal(a[b, t, :n[b, t]].view(np.int32), c[b, t, :n[b, t]].view(np.int32)), "two runs differ"
    assert np.array_equal(got[3], again[3])


def test_unmerged_and_reference_layout():
    """merge=False leaves z and the labels per task; swapped=False reads a transposed map to the same detections."""
    h, chan, _, _, p = cases.make("circle_128_b1")
    ref = C.postprocess(h, cases.NUSC_TASKS, chan, **dict(p, merge=False))
    _compare(_run_kernel(h, chan, dict(p, merge=False)), ref, "unmerged")
    # the same scene as a [x, y] map.  Ties cannot occur (planted scores are distinct), so the flat-index rule is idle
    ht = np.ascontiguousarray(h.transpose(0, 2, 1, 3))
    got = _run_kernel(ht, chan, dict(p, merge=False, swapped=False))
    _compare(got, ref, "reference layout")


def test_max_num_above_cells_raises():
    from al3d import detector_ops as D, lib
    h, chan, _, _, p = cases.make("circle_128_b1")
    small = torch.from_numpy(np.ascontiguousarray(h[:, :20, :20])).cuda()
    with pytest.raises(lib.Al3dError, match="exceeds"):
        D.center_decode_nms(small, cases.NUSC_TASKS, chan, **p)


def _grouped_ref(x, w, bias, cout, coff, ldc):
    """float64 grouped convolution + the bound's sum of magnitudes, via torch conv2d in float64 on the CPU."""
    B, H, W, C = x.shape
    out = np.zeros((B, H, W, ldc))
    mag = np.zeros((B, H, W, ldc))
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    row = 0
    for g, (co, off) in enumerate(zip(cout, coff)):
        wg = torch.from_numpy(w[row:row + co]).double().reshape(co, 3, 3, 64).permute(0, 3, 1, 2)
        bg = torch.from_numpy(bias[row:row + co]).double()
        xg = xt[:, g * 64:(g + 1) * 64]
        out[..., off:off + co] = torch.nn.functional.conv2d(xg, wg, bg, padding=1).permute(0, 2, 3, 1).numpy()
        mag[..., off:off + co] = torch.nn.functional.conv2d(xg.abs(), wg.abs(), bg.abs(), padding=1).permute(0, 2, 3, 1).numpy()
        row += co
    return out, mag


@pytest.mark.parametrize("G,couts,H,W", [(1, [8], 7, 9), (6, [2, 1, 3, 2, 2, 2], 13, 11), (36, None, 9, 5), (3, [1, 8, 3], 31, 33),
                                            (3, [4, 5, 7], 6, 10), (2, [6, 4], 5, 5)])
def test_grouped_conv_matches_float64(G, couts, H, W):
    """Bound: an output is bias + 576 sequential float32 FMAs; the classic running-sum bound gives
    |error| <= 577 * u * (|bias| + sum |x| |w|), u = 2^-24, evaluated per output in float64."""
    from al3d import detector_ops as D
    rng = np.random.default_rng(G)
    couts = couts or [int(c) for c in rng.integers(1, 4, G)]
    B = 2
    x = rng.normal(0, 1, (B, H, W, G * 64)).astype(np.float32)
    w = rng.normal(0, 0.1, (sum(couts), 9, 64)).astype(np.float32)
    bias = rng.normal(0, 1, sum(couts)).astype(np.float32)
    coff, o = [], 1                                         # a gap before, between and after the windows
    for c in couts:
        coff.append(o)
        o += c + 1
    out = torch.full((B, H, W, o), 7.0, device="cuda")
    D.conv3x3_grouped_nhwc(torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(bias).cuda(), couts, coff, out=out)
    got = out.cpu().numpy().astype(np.float64)
    ref, mag = _grouped_ref(x, w, bias, couts, coff, o)
    written = np.zeros(o, bool)
    for c, off in zip(couts, coff):
        written[off:off + c] = True
    assert np.all(got[..., ~written] == 7.0), "the kernel wrote outside its channel windows"
    err = np.abs(got - ref)[..., written]
    print("grouped conv: max error", err.max(), "max error / bound", (err / (577 * U * mag[..., written])).max())
    assert np.all(err <= 577 * U * mag[..., written])


HEAD_CFG = dict(
    type="CenterHead", in_channels=32, share_conv_channel=64, norm_bbox=True, transpose_input=True,
    tasks=[["car"], ["truck", "construction_vehicle"], ["pedestrian", "traffic_cone"]],
    common_heads=dict(reg=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2], vel=[2, 2]),
    separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3),
    bbox_coder=dict(type="CenterPointBBoxCoder", pc_range=[-54.0, -54.0], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                    max_num=100, score_threshold=0.1, out_size_factor=8, voxel_size=[0.075, 0.075], code_size=9),
    test_cfg=dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], min_radius=[4, 12, 0.175], score_threshold=0.1,
                  nms_type=["rotate", "rotate", "circle"], pre_max_size=1000, post_max_size=83, nms_thr=0.2))


def _head(seed=0, device="cuda", **over):
    from al3d import synthetic
    from al3d.models import build_head
    head = build_head(dict(HEAD_CFG, **over))
    synthetic.seeded_init_(head, seed=seed)
    return head.to(device).eval()


def _torch_forward(head, x_nhwc):
    """The reference graph in float64 NCHW torch ops on the reference's [x, y] map (the head runs with transpose_input)."""
    import torch.nn.functional as F
    x = x_nhwc.double().permute(0, 3, 2, 1)                                  # [B, C, x, y]

    def cm(m, v):
        v = F.conv2d(v, m.conv.weight.double(), None, padding=1)
        return F.relu(F.batch_norm(v, m.bn.running_mean.double(), m.bn.running_var.double(), m.bn.weight.double(), m.bn.bias.double(),
                                   False, 0.0, m.bn.eps))
    feat = cm(head.shared_conv, x)
    out = []
    for th in head.task_heads:
        out.append({h: F.conv2d(cm(getattr(th, h)[0], feat), getattr(th, h)[1].weight.double(), getattr(th, h)[1].bias.double(), padding=1)
                    for h in th.heads})
    return out


def test_head_forward_matches_torch_and_is_deterministic():
    head = _head()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 22, 26, 32, generator=g).cuda()                       # [B, H = y, W = x, C], non-square
    with torch.no_grad():
        preds = head(x)
        ref = _torch_forward(head, x)
        again = head(x)
    assert torch.equal(preds.fused, again.fused), "two runs differ"
    for t, (p, r) in enumerate(zip(preds, ref)):
        for h in r:
            got = p[0][h].double().permute(0, 1, 3, 2)                       # [B, C, y, x] -> [B, C, x, y]
            scale = r[h].abs().max().item()
            err = (got - r[h]).abs().max().item()
            print(f"task {t} {h}: max error {err:.3e} of scale {scale:.3e}")
            assert err <= 1e-4 * scale
    with torch.no_grad():
        dets = head.get_bboxes(preds)
        dets2 = head.get_bboxes(again)
    assert len(dets) == 2
    for a, b in zip(dets, dets2):
        assert a["bboxes"].shape[1] == 9 and a["bboxes"].dtype == torch.float32 and a["labels"].dtype == torch.int64
        assert a["bboxes"].shape[0] == a["scores"].shape[0] == a["labels"].shape[0]
        assert all(torch.equal(a[k], b[k]) for k in a)


def _head_params(head):
    from al3d import detector_ops as D
    _, spans = head._layout()
    chan = [[sp[h][0] if h in sp else -1 for h in D.CENTER_CHANNELS] for sp in spans]
    c, tc = head.bbox_coder, head.test_cfg
    F32 = cases.F32
    p = dict(swapped=False, max_num=c["max_num"], norm_bbox=True, out_size_factor=8.0, voxel_size=[F32(0.075)] * 2, pc_range=c["pc_range"],
             coder_score_threshold=F32(0.1), post_center_range=c["post_center_range"], nms_type=tc["nms_type"],
             nms_scale=[[1.0] * n for n in head.num_classes], min_radius=tc["min_radius"], score_threshold=F32(0.1), nms_thr=F32(0.2),
             pre_max_size=1000, post_max_size=83, post_center_limit_range=tc["post_center_limit_range"], merge=True)
    return chan, spans, p


DET_SEED = 5      # chosen on the CPU (float64 evaluation only) so that the margins asserted below hold


def _detection_case(device):
    """The seeded head and input of the detection test, and the float64 evaluation of the reference graph + float64
    post-processing on the reference's [x, y] maps: (head, x, ref maps, ref detections, margins).  Margins: the smallest
    distance of a candidate score from the score threshold, the smallest gap between two scores above it (their order),
    and the smallest distance of an NMS quantity from its threshold."""
    head = _head(seed=DET_SEED, device=device, bbox_coder=dict(HEAD_CFG["bbox_coder"], max_num=20))
    g = torch.Generator().manual_seed(DET_SEED)
    x = torch.randn(2, 22, 26, 32, generator=g).to(device)
    with torch.no_grad():
        # seeded weights saturate the heat map (every score near 1, gaps of 1e-6): rescale each task's last heat-map layer
        # so that its logits have standard deviation 1.5 about -2: scores spread over (0, 1), most below the threshold
        for th, m in zip(head.task_heads, _torch_forward(head, x)):
            mean, std = m["heatmap"].mean().item(), m["heatmap"].std().item()
            th.heatmap[1].weight.mul_(1.5 / std)
            th.heatmap[1].bias.copy_((th.heatmap[1].bias - mean) * (1.5 / std) - 2.0)
        maps = _torch_forward(head, x)
    chan, spans, p = _head_params(head)
    hout = torch.cat([m[h] for m, sp in zip(maps, spans) for h in sp], dim=1).permute(0, 2, 3, 1).cpu().numpy()      # [B, x, y, CH]
    pairs = {}
    ref = C.postprocess(hout, head.num_classes, chan, pairs=pairs, **p)
    thr_margin, gap, nms_margin = np.inf, np.inf, np.inf
    for b, row in enumerate(ref):
        for t, r in enumerate(row):
            s = r["decoded"]["all_scores"]
            thr_margin = min(thr_margin, np.abs(s - p["score_threshold"]).min())
            # order and membership of the top-K: the K + 1 best scores of every class of the task, all together
            heat = C.sigmoid(maps[t]["heatmap"][b].reshape(head.num_classes[t], -1).cpu().numpy())
            top = np.sort(np.concatenate([np.sort(c)[-(p["max_num"] + 1):] for c in heat]))
            gap = min(gap, np.diff(top).min())
            lim = p["nms_thr"] if p["nms_type"][t] == "rotate" else p["min_radius"][t]
            for _, _, q in pairs.get((b, t), ()):
                nms_margin = min(nms_margin, abs(q - lim))
            xyz = r["decoded"]["all_boxes"][s > p["score_threshold"], :3]
            for rng6 in (p["post_center_range"], p["post_center_limit_range"]):
                if len(xyz):
                    nms_margin = min(nms_margin, np.abs(xyz[:, None, :] - np.asarray(rng6).reshape(2, 3)[None]).min())
    return head, x, maps, ref, (thr_margin, gap, nms_margin), spans


def test_head_detections_equal_independent_evaluation():
    """``forward`` + ``get_bboxes`` against the float64 NCHW torch evaluation of the same parameters fed through the float64
    post-processing: equal counts, order and labels; scores and boxes within what a map error of e = 1e-4 of each map's
    scale (the tolerance of the map comparison above) can move them:
      score: s (1 - s) e_heat + 4u;  x, y: 0.6 e_reg + 4u * 128;  dim: relative e_dim (1 + e_dim) + 4u;
      z = height - dim2 / 2: e_height + dim2 e_dim + 16u;  rot = atan2(a, b): sqrt(2) e_rot / hypot(a, b) + 3 * 2^-22;  vel: e_vel.
    No sample is excused: seed and heat-map bias are fixed so that, in float64, every candidate score is at least 1e-4 from
    the threshold, two scores above it at least 1e-4 apart and every NMS quantity (IoU, squared distance, centre) at least
    1e-3 from its threshold -- 100 times the flips a 1e-6 map error (measured: 2e-6 of scale) could cause; asserted."""
    head, x, maps, ref, (thr_margin, gap, nms_margin), spans = _detection_case("cuda")
    print(f"margins: score threshold {thr_margin:.3e}, score gap {gap:.3e}, nms / range {nms_margin:.3e}")
    assert thr_margin >= 1e-4 and gap >= 1e-4 and nms_margin >= 1e-3, "the fixed seed no longer keeps the case off the thresholds"
    with torch.no_grad():
        dets = head.get_bboxes(head(x))
    e = [{h: 1e-4 * m[h].abs().max().item() for h in m} for m in maps]
    compared = 0
    for b, row in enumerate(ref):
        want_s = np.concatenate([r["scores"] for r in row])
        want_b = np.concatenate([r["boxes"] for r in row])
        got_b = dets[b]["bboxes"].cpu().numpy().astype(np.float64)
        print(f"sample {b}: float64 {len(want_s)} detections per task {[len(r['scores']) for r in row]}, device {len(got_b)}")
        assert len(got_b) == len(want_s)
        assert np.array_equal(dets[b]["labels"].cpu().numpy(), np.concatenate([r["labels"] for r in row]))
        et = np.concatenate([np.full(len(r["scores"]), t) for t, r in enumerate(row)]).astype(int)
        eh = lambda h: np.array([e[t][h] for t in et])                        # noqa: E731
        assert np.all(np.abs(dets[b]["scores"].cpu().numpy() - want_s) <= want_s * (1 - want_s) * eh("heatmap") * 1.01 + 4 * U)
        err = np.abs(got_b - want_b)
        # raw rot channels of each detection, for the atan2 bound
        rv = np.concatenate([maps[t]["rot"][b].reshape(2, -1)[:, torch.as_tensor(r["cells"], device=maps[t]["rot"].device)].cpu().numpy().T
                             for t, r in enumerate(row)])
        assert np.all(err[:, :2] <= 0.6 * eh("reg")[:, None] + 4 * U * 128)
        assert np.all(err[:, 3:6] <= want_b[:, 3:6] * (eh("dim") * (1 + eh("dim")) + 4 * U)[:, None])
        assert np.all(err[:, 2] <= eh("height") + want_b[:, 5] * eh("dim") + 16 * U)
        assert np.all(err[:, 6] <= np.sqrt(2) * eh("rot") / np.hypot(rv[:, 0], rv[:, 1]) + 3 * 2.0 ** -22)
        assert np.all(err[:, 7:] <= eh("vel")[:, None])
        compared += len(want_s) > 0
    assert compared >= 1, "no sample with detections was compared"


def test_no_detections_gives_empty_tensors_and_7_value_boxes():
    head = _head(seed=1, common_heads=dict(reg=[2, 2], height=[1, 2], dim=[3, 2], rot=[2, 2]))
    with torch.no_grad():
        for th in head.task_heads:
            th.heatmap[1].weight.zero_()
            th.heatmap[1].bias.fill_(-10.0)
        out = head.predict(dict(metadata=["a", "b"]), head(torch.randn(2, 16, 20, 32).cuda()))
    assert [o["metadata"] for o in out] == ["a", "b"]
    for o in out:
        assert o["box3d_lidar"].shape == (0, 7) and o["box3d_lidar"].dtype == torch.float32
        assert o["scores"].shape == (0,) and o["scores"].dtype == torch.float32
        assert o["label_preds"].shape == (0,) and o["label_preds"].dtype == torch.int64


def test_host_reads_the_counts_once_and_nothing_else():
    """Asserted with torch.cuda.set_sync_debug_mode("error") from ``forward`` to the end of ``get_bboxes``; the one read
    of the counts (``CenterHead._read_counts``) is counted and exempted."""
    head = _head()
    x = torch.randn(2, 16, 20, 32).cuda()
    with torch.no_grad():
        head.get_bboxes(head(x))                                              # warm-up: packs the weights (host work)
    calls = []
    plain = type(head)._read_counts

    def read(counts):
        calls.append(1)
        torch.cuda.set_sync_debug_mode("default")
        try:
            return plain(counts)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    head._read_counts = read
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            dets = head.get_bboxes(head(x))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(calls) == 1 and len(dets) == 2
