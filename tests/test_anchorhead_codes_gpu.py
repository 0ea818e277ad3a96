"""GPU suite of ``al3d_head_decode_nms_codes`` / ``al3d_box_decode_codes_f32`` (csrc/head_nms.hip) and of ``MultiGroupHead``
with the direction classifier: the reference's own ``predict`` goldens (tests/golden/head_predict_codes.npz) through the C-ABI
and through the module, the planted exact edges of the fix-up against torch's float32 arithmetic, the stand-alone decode, the
10-wide vector code through the new entry against the old entry bit for bit, odd and unaligned records, B = 1 and one task,
and det3d's PointPillars with this head end to end.  Shapes, cases and tolerances: tests/anchorhead_codes.py.

Kernel instantiations launched here: head_nms_kernel<7,0,true> (s7_dir, edges), <9,0,true> (s9_dir, s9_nodir with every
dir_off -1, edges, end to end), <7,1,true> (v7_dir), <9,1,true> (v9_dir), <9,1,false> through both entries; the four
box_decode_codes_kernel<ND,VEC>."""
import os

import numpy as np
import pytest
import torch

import anchorhead_codes as AX

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["s7_dir", "s9_dir", "v7_dir", "s9_nodir", "v9_dir"]


@pytest.mark.parametrize("name", NAMES)
def test_codes_entry_equals_the_reference_head(name):
    c = AX.load(name)
    got = AX.run_codes(c, AX.fused(c))
    assert got[3][1, 1] == 0                                       # the (sample, task) without a candidate
    for b in range(c["B"]):
        AX.assert_close(AX.merged(got, b), c["ref"][b], f"{name} sample {b}")


def _module(c):
    from al3d.models.bbox_heads import MultiGroupHead
    from al3d.models.box_coder import GroundBox3dCoderTorch
    tasks = [dict(num_class=1, class_names=["car"]), dict(num_class=2, class_names=["motorcycle", "bicycle"])]
    aux = dict(type="WeightedSoftmaxClassificationLoss", name="direction_classifier") if c["with_dir"] else None
    return MultiGroupHead(in_channels=16, tasks=tasks, box_coder=GroundBox3dCoderTorch(False, bool(c["vec"]), n_dim=c["n_dim"]),
                          loss_aux=aux, direction_offset=c["offset"]).cuda().eval()


def _module_predict(c, m, defer=False):
    hout, box_off, cls_off, dir_off = AX.fused(c)
    assert (box_off, cls_off, dir_off, hout.shape[2]) == (m._box_off, m._cls_off, m._dir_off, m._ch)
    p = c["params"]
    cfg = dict(score_threshold=p["score_thresh"], post_center_limit_range=p["rng"],
               nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=p["pre_max"],
                        nms_post_max_size=p["post_max"], nms_iou_threshold=p["iou_thresh"]))
    fused = torch.from_numpy(hout).cuda().view(c["B"], c["H"], c["W"], -1)
    ex = {"anchors": [torch.from_numpy(np.broadcast_to(a, (c["B"],) + a.shape).copy()) for a in c["anchors"]],
          "metadata": [{"token": b} for b in range(c["B"])]}
    m.defer_nms = defer
    return m.predict(ex, [{"_fused": fused}], cfg)


@pytest.mark.parametrize("name", NAMES)
def test_module_predict_equals_the_reference_head(name):
    from al3d.models.bbox_heads import LazyDetections
    c = AX.load(name)
    m = _module(c)
    det = _module_predict(c, m)
    assert isinstance(det, LazyDetections) and len(det) == c["B"]
    for b in range(c["B"]):
        d = det[b]
        assert d["box3d_lidar"].shape[1] == c["n_dim"] and d["label_preds"].dtype == torch.int64 and d["metadata"] == {"token": b}
        AX.assert_close(dict(boxes=d["box3d_lidar"].cpu().numpy(), scores=d["scores"].cpu().numpy(),
                             labels=d["label_preds"].cpu().numpy()), c["ref"][b], f"{name} sample {b}")


@pytest.mark.parametrize("name", ["s7_dir", "v9_dir"])
def test_module_forward_carries_the_direction_logits(name):
    """The fused 1x1 launch [all box | all class | all dir] against the separate Conv2d of the reference's Head.forward, and
    ``predict`` on that launch's own output against the numpy restatement on the same buffer."""
    import torch.nn.functional as F
    from al3d import synthetic
    from al3d.models.bbox_heads import MultiGroupHead
    from al3d.models.box_coder import GroundBox3dCoderTorch
    c = AX.load(name)
    tasks = [dict(num_class=1, class_names=["car"]), dict(num_class=2, class_names=["motorcycle", "bicycle"])]
    m = MultiGroupHead(in_channels=64, tasks=tasks, box_coder=GroundBox3dCoderTorch(False, bool(c["vec"]), n_dim=c["n_dim"]),
                       loss_aux=dict(type="WeightedSoftmaxClassificationLoss", name="direction_classifier"),
                       direction_offset=c["offset"])
    synthetic.seeded_init_(m, seed=5)
    m = m.cuda().eval()
    x = torch.randn(c["B"], c["H"], c["W"], 64, generator=torch.Generator().manual_seed(9)).cuda()
    with torch.no_grad():
        preds = m(x)
    xn = x.permute(0, 3, 1, 2).cpu()
    for t, task in enumerate(m.tasks):
        for key, conv in (("box_preds", task.conv_box), ("cls_preds", task.conv_cls), ("dir_cls_preds", task.conv_dir)):
            ref = F.conv2d(xn, conv.weight.detach().cpu(), conv.bias.detach().cpu()).permute(0, 2, 3, 1)
            assert preds[t][key].shape == ref.shape
            torch.testing.assert_close(preds[t][key].cpu(), ref, rtol=1e-4, atol=1e-4)
    fused = preds[0]["_fused"]
    assert fused.shape[-1] == m._ch and preds[1]["dir_cls_preds"].data_ptr() == fused[..., m._dir_off[1]:].data_ptr()
    p = c["params"]
    cfg = dict(score_threshold=p["score_thresh"], post_center_limit_range=p["rng"],
               nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=p["pre_max"],
                        nms_post_max_size=p["post_max"], nms_iou_threshold=p["iou_thresh"]))
    det = m.predict({"anchors": [torch.from_numpy(a) for a in c["anchors"]]}, preds, cfg)
    hout = fused.cpu().numpy().reshape(c["B"], c["H"] * c["W"], -1)
    want = AX.predict(c, (hout, m._box_off, m._cls_off, m._dir_off))
    assert sum(len(w["labels"]) for w in want) > 10
    for b in range(c["B"]):
        d = det[b]
        AX.assert_close(dict(boxes=d["box3d_lidar"].cpu().numpy(), scores=d["scores"].cpu().numpy(),
                             labels=d["label_preds"].cpu().numpy()), want[b], f"{name} forward sample {b}")


def test_module_defer_nms_holds_the_launch_back():
    c = AX.load("s9_dir")
    m = _module(c)
    det = _module_predict(c, m, defer=True)
    assert det._raw_ is None and len(det) == c["B"]
    m.flush_deferred()
    assert det._raw_ is not None
    AX.assert_close(dict(boxes=det[0]["box3d_lidar"].cpu().numpy(), scores=det[0]["scores"].cpu().numpy(),
                         labels=det[0]["label_preds"].cpu().numpy()), c["ref"][0], "deferred")


@pytest.mark.parametrize("n_dim,offset", [(7, 0.78), (9, 0.78), (7, 0.0), (9, 0.0)])
def test_planted_edges_equal_torch_exactly(n_dim, offset):
    case, layout, plants = AX.edge_case(n_dim, offset)
    r, opp, mask = AX.edge_expected(plants, offset, n_dim)
    boxes, scores, labels, counts = AX.run_codes(case, layout)
    k = int(counts[0, 0])
    kept = [p for p, m in zip(plants, mask) if m]
    assert k == len(kept) == len(plants) - 1
    xs = [float(case["anchors"][0][p[1], 0]) for p in kept]
    ys = [float(case["anchors"][0][p[1], 1]) for p in kept]
    assert boxes[0, 0, :k, 0].tolist() == xs and boxes[0, 0, :k, 1].tolist() == ys         # the plants, in score order
    want = r[mask]
    got = boxes[0, 0, :k, n_dim - 1]
    for p, g, w in zip(kept, got, want):
        assert np.float32(g).view(np.int32) == np.float32(w).view(np.int32), (p[0], float(g), float(w))
    assert boxes[0, 0, :k, 2].tolist() == [float(p[4]) for p in kept]                    # z == range[5] stays, flipped or not
    assert np.all(boxes[0, 0, k:] == AX.SENTINEL)
    # the same plants without the classifier: the decoded angle itself
    plain = AX.run_codes(case, (layout[0], layout[1], layout[2], [-1]))
    assert plain[0][0, 0, :k, n_dim - 1].tolist() == [float(p[2]) for p in kept]
    assert np.array_equal(plain[1], scores) and np.array_equal(plain[2], labels) and np.array_equal(plain[3], counts)
    assert np.array_equal(plain[0][..., :n_dim - 1], boxes[..., :n_dim - 1])


def _second_box_decode(enc, anchors, vec):
    """torch restatement of second_box_decode (box_torch_ops.py:80-148), float32 on the CPU."""
    nd = anchors.shape[-1]
    a = torch.split(anchors, 1, dim=-1)
    t = torch.split(enc, 1, dim=-1)
    xa, ya, za, wa, la, ha, ra = a[0], a[1], a[2], a[3], a[4], a[5], a[-1]
    diagonal = torch.sqrt(la ** 2 + wa ** 2)
    ret = [t[0] * diagonal + xa, t[1] * diagonal + ya, t[2] * ha + za,
           torch.exp(t[3]) * wa, torch.exp(t[4]) * la, torch.exp(t[5]) * ha]
    if nd == 9:
        ret.extend([t[6] + a[6], t[7] + a[7]])
    if vec:
        ret.append(torch.atan2(t[nd] + torch.sin(ra), t[nd - 1] + torch.cos(ra)))
    else:
        ret.append(t[nd - 1] + ra)
    return torch.cat(ret, dim=-1)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("n_dim,vec", [(7, 0), (9, 0), (7, 1), (9, 1)])
def test_standalone_decode(n_dim, vec, n):
    import ctypes
    from al3d import lib
    rng = np.random.default_rng(100 * n_dim + 10 * vec + n)
    enc = rng.normal(0, 0.4, (n, n_dim + vec)).astype(np.float32)
    anc = np.zeros((n, n_dim), np.float32)
    anc[:, :3] = rng.uniform(-50, 50, (n, 3))
    anc[:, 3:6] = rng.uniform(0.4, 12.0, (n, 3))
    anc[:, 6:n_dim - 1] = rng.normal(0, 2, (n, n_dim - 7))
    anc[:, n_dim - 1] = rng.choice([0.0, 1.57], n)
    ref = _second_box_decode(torch.from_numpy(enc), torch.from_numpy(anc), vec).numpy().astype(np.float64)
    e, a = torch.from_numpy(enc).cuda(), torch.from_numpy(anc).cuda()
    out = torch.full((n + 1, n_dim), AX.SENTINEL, dtype=torch.float32, device="cuda")
    vp = lambda x: ctypes.c_void_p(x.data_ptr())      # noqa: E731
    lib.call("al3d_box_decode_codes_f32", vp(e), vp(a), n, n_dim, vec, vp(out), torch.cuda.current_stream().cuda_stream)
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(got[n] == AX.SENTINEL)
    np.testing.assert_allclose(got[:n, :-1], ref[:, :-1], rtol=2e-6, atol=2e-6)
    d = np.abs(got[:n, -1] - ref[:, -1])
    assert np.minimum(d, np.abs(2 * np.pi - d)).max() < 1e-5
    if n_dim == 9 and vec:                            # the old stand-alone decode is the same code
        old = torch.empty((n, 9), dtype=torch.float32, device="cuda")
        lib.call("al3d_box_decode_f32", vp(e), vp(a), n, vp(old), torch.cuda.current_stream().cuda_stream)
        assert torch.equal(old.view(torch.int32), out[:n].view(torch.int32))


def test_vector_code_without_classifier_is_the_old_entry_bit_for_bit():
    c = AX.load("v9_dir")
    layout = AX.fused(c, with_dir=False)
    new = AX.run_codes(c, layout)
    old = AX.run_codes(c, layout, old_entry=True)
    assert int(new[3].sum()) > 20
    for g, o in zip(new, old):
        assert np.array_equal(g.view(np.int32), o.view(np.int32))
    # and with the classifier's logits present but switched off (every dir_off -1) nothing else moves
    hout, box_off, cls_off, _ = AX.fused(c)
    off = AX.run_codes(c, (hout, box_off, cls_off, [-1, -1]))
    for g, o in zip(off, old):
        assert np.array_equal(g.view(np.int32), o.view(np.int32))


def test_refusals_on_the_gpu_box():
    got = AX.refusals()
    assert len(got) == 8 and all(rc == -1 for _, rc, _ in got), got


@pytest.mark.parametrize("name", ["s7_dir", "s9_dir", "v7_dir", "s9_nodir"])
def test_odd_record_and_unaligned_direction_window(name):
    c = AX.load(name)
    layout = AX.odd_layout(c)
    assert layout[0].shape[2] % 2 == 1 and layout[2][0] % 4 != 0
    if name in ("s7_dir", "s9_dir"):
        assert layout[3][0] % 4 != 0
    got = AX.run_codes(c, layout)
    for b in range(c["B"]):
        AX.assert_close(AX.merged(got, b), c["ref"][b], f"{name} sample {b}")


def _task_of(c, ref, t):
    lo = int(np.sum(c["nc"][:t]))
    sel = (ref["labels"] >= lo) & (ref["labels"] < lo + c["nc"][t])
    return dict(boxes=ref["boxes"][sel], scores=ref["scores"][sel], labels=ref["labels"][sel] - lo)


@pytest.mark.parametrize("name", ["s7_dir", "v9_dir"])
def test_one_sample_and_one_task(name):
    c = AX.load(name)
    hout, box_off, cls_off, dir_off = AX.fused(c)
    for b in range(c["B"]):                           # B = 1, both tasks
        one = dict(c, B=1)
        got = AX.run_codes(one, (np.ascontiguousarray(hout[b:b + 1]), box_off, cls_off, dir_off))
        AX.assert_close(AX.merged(got, 0), c["ref"][b], f"{name} sample {b} alone")
    for t in range(2):                                # ntasks = 1, both samples
        one = dict(c, nc=[c["nc"][t]], na=[c["na"][t]], anchors=[c["anchors"][t]])
        got = AX.run_codes(one, (hout, [box_off[t]], [cls_off[t]], [dir_off[t]]))
        for b in range(c["B"]):
            AX.assert_close(AX.merged(got, b), _task_of(c, c["ref"][b], t), f"{name} task {t} alone, sample {b}")


def test_prepass_matching_takes_seven_wide_boxes():
    """The PPAL / CALD matching pre-pass on this head's raw 7-wide buffers: matched against its own detections every kept
    box finds itself (scale IoU 1)."""
    c = AX.load("s7_dir")
    det = _module_predict(c, _module(c))
    ref_boxes = torch.from_numpy(np.concatenate([r["boxes"] for r in c["ref"]])).cuda()
    ref_labels = torch.from_numpy(np.concatenate([r["labels"] for r in c["ref"]]).astype(np.int32)).cuda()
    ref_scores = torch.from_numpy(np.concatenate([r["scores"] for r in c["ref"]])).cuda()
    ref_off = torch.tensor(np.concatenate([[0], np.cumsum([len(r["labels"]) for r in c["ref"]])]), dtype=torch.int32).cuda()
    out = det.match((ref_boxes, ref_labels, ref_scores, ref_off), ncls=3, dist_th=0.5)
    counts = det._raw[3].cpu().numpy()
    iou = out["match_iou"].cpu().numpy()
    ref = out["match_ref"].cpu().numpy()
    for b in range(c["B"]):
        for t in range(2):
            k = counts[b, t]
            assert np.all(ref[b, t, :k] >= 0) and np.all(np.abs(iou[b, t, :k] - 1.0) < 1e-5)
    assert out["cls_count"].cpu().numpy().sum() == counts.sum() == sum(len(r["labels"]) for r in c["ref"])
    ent = det.frame_entropy().cpu().numpy()
    for b in range(c["B"]):
        s = torch.from_numpy(c["ref"][b]["scores"])
        np.testing.assert_allclose(ent[b], (-s * torch.log(s) - (1.0 - s) * torch.log(1 - s)).mean().item(), rtol=2e-6)


def _example_model():
    """The example config's detector with seeded weights.  The seeded class convs saturate every kept score at exactly 1.0
    (entropy 0 * -inf = NaN, in the reference's formula too), so they are scaled down to spread the scores over (0.1, 1)."""
    from al3d import synthetic
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "pointpillars_mghead_entropy.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    with torch.no_grad():
        for t in model.bbox_head.tasks:
            t.conv_cls.weight.mul_(0.02)
            t.conv_cls.bias.fill_(-1.5)
    return cfg, model


def test_example_config_runs_through_the_selection_cli(tmp_path):
    """examples/active/pointpillars_mghead_entropy.py through tools/active_select.py on an on-disk synthetic pool (the
    file-fed loader with the padded point slots) with a checkpoint that carries ``conv_dir``: the bootstrap run, then sweep +
    selection."""
    import json
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from write_synthetic_pool import write_pool
    root = str(tmp_path / "pool")
    infos, _ = write_pool(root, scenes=1, base=2)
    cfg = tmp_path / "cfg.py"
    cfg.write_text(f'_base_ = "{os.path.join(ROOT, "examples", "active", "pointpillars_mghead_entropy.py")}"\n'
                   f'data_root = "{root}"\n'
                   f'selector = dict(infos_origin="{root}/infos.pkl", buffer_file="{tmp_path}/buffers/pp.json", '
                   f'buffer_path="{tmp_path}/buffers/entropy_pred.pt")\n')
    _, model = _example_model()
    sd = model.state_dict()
    assert "bbox_head.tasks.5.conv_dir.weight" in sd
    torch.save({"state_dict": sd}, tmp_path / "ckpt.pth")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "active_select.py"), "--config", str(cfg), "--budget", "10", "--pred",
           "--batch", "8", "--checkpoint", str(tmp_path / "ckpt.pth")]
    for _ in range(2):
        r = subprocess.run(cmd, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
    out = json.load(open(tmp_path / "buffers" / "pp.json"))
    assert list(out) == ["0", "10"] and len(out["10"]) >= 1 and len(set(out["10"])) == len(out["10"])
    ent = torch.load(tmp_path / "buffers" / "entropy_pred.pt", weights_only=True)
    assert ent.shape[0] == len(infos) and bool(torch.isfinite(ent).all()) and bool((ent > 0.05).all())
    assert "missing 0, unexpected 0" in r.stderr


def test_pointpillars_with_the_anchor_head_end_to_end():
    from al3d.datasets import DeviceSweepLoader, PoolFrames, generate_task_anchors
    dev = torch.device("cuda:0")
    cfg, model = _example_model()
    model = model.to(dev).eval()
    assert model.bbox_head.use_direction_classifier and model.bbox_head._codes_entry
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])
    pool = PoolFrames.from_synthetic(2, dev, seed=1000)
    loader = DeviceSweepLoader(pool, cfg.voxel_generator, anchors, batch_size=2, device=dev, with_points=True)
    with torch.no_grad():
        preds, middle = model(next(iter(loader)), return_loss=False, estimate=True)
    assert len(preds) == 2 and tuple(middle[-1].shape) == (2, 384, 128, 128)
    ent = preds.frame_entropy().cpu().numpy()
    total = 0
    for b in range(2):
        d = preds[b]
        k = d["scores"].shape[0]
        total += k
        assert d["box3d_lidar"].shape == (k, 9) and bool(torch.isfinite(d["box3d_lidar"]).all())
        assert bool(((d["scores"] >= 0.1) & (d["scores"] <= 1)).all()) and int(d["label_preds"].max()) < 10
        s = d["scores"].cpu()
        assert np.isfinite(ent[b]) and ent[b] > 0.05 and float(s.max()) < 1.0
        np.testing.assert_allclose(ent[b], (-s * torch.log(s) - (1.0 - s) * torch.log(1 - s)).mean().item(), rtol=2e-6)
    assert total > 0
