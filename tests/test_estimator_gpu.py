"""GPU suite for the box-wise IoU estimator (csrc/estimator.hip, ``selector_ops.estimate_boxes``, ``models.Estimator``,
``models.WithEstimator``) on the inputs of tests/golden/estimator.npz, against the float64 values stored there (the
restatement tests/estimator_numpy.py, which tests/test_estimator_cpu.py pins to the reference's own run).  Never against
the kernel's own output.

Tolerances: per-box point counts, surviving slots, new counts: equal (the generator keeps every point 1e-3 m away from
every membership boundary).  Boxes and labels of the survivors: the input's bits.  IoUs and pooled rows: 4 x
``ref_f32_gap``, the reference's own float32 distance from float64 on this fixture, read from the file.  The entropy of a
frame: the IoU tolerance carried through the largest slope |log((1 - p) / p)| of the binary entropy at the frame's golden
IoUs, plus the 2e-6 relative of the entropy kernel's own gate (tests/test_selector_edges_cpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import estimator_numpy as EN

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = [dict(num_class=4, class_names=["a", "b", "c", "d"]), dict(num_class=6, class_names=list("efghij"))]
CHILD_LIMIT_S = 240
FAULT_CODES = (124, 134, 137, 139)
_faulted = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "estimator.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def module(z, dev):
    from al3d.models import build_estimator
    m = build_estimator(dict(type="Estimator", tasks=TASKS, dim_feat=224))
    m.load_state_dict({k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("state.")}, strict=True)
    return m.to(dev).eval()


def inputs(z, dev):
    t = lambda k, d: torch.from_numpy(np.ascontiguousarray(z[k], dtype=d)).to(dev)      # noqa: E731
    return dict(boxes=t("boxes", np.float32), scores=t("scores", np.float32), labels=t("labels", np.int32),
                counts=t("counts", np.int32), points=t("points", np.float32), offsets=t("offsets", np.int64))


def run(z, dev, module, **kw):
    from al3d import selector_ops as ops
    i = inputs(z, dev)
    res = ops.estimate_boxes(i["boxes"], i["labels"], i["counts"], i["points"], i["offsets"],
                             module.packed_weights(dev), module.num_classes, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.fixture(scope="module")
def got(z, dev, module):
    return run(z, dev, module)


def survivors(z):
    """[(b, t, source slot, destination slot)] of the golden."""
    out = []
    B, nt, post = z["ref_survivor_mask"].shape
    for b in range(B):
        for t in range(nt):
            for r, i in enumerate(np.nonzero(z["ref_survivor_mask"][b, t])[0]):
                out.append((b, t, int(i), r))
    return out


def test_point_counts_exact(z, got):
    valid = np.arange(8)[None, None, :] < z["counts"][:, :, None]
    assert np.array_equal(got["npts"][valid], z["ref_npts"][valid])
    assert (got["npts"][~valid] == 0).all()                 # slots behind the counts are never tested
    assert int(got["status"][0]) == 0


def test_survivors_and_counts_exact(z, got):
    assert np.array_equal(got["counts"], z["ref_out_counts"])
    assert got["counts"].sum() == 12 and got["counts"][1:].sum() == 0      # frames 1..3 come back empty, no error
    for b, t, src, dst in survivors(z):
        assert np.array_equal(got["boxes"][b, t, dst].view(np.int32), z["boxes"][b, t, src].view(np.int32))
        assert got["labels"][b, t, dst] == z["labels"][b, t, src]


def test_ious_and_pooled_rows_within_the_reference_gap(z, got):
    tol = 4 * float(z["ref_f32_gap"])
    worst_iou = worst_pool = 0.0
    for b, t, src, dst in survivors(z):
        worst_iou = max(worst_iou, abs(float(got["scores"][b, t, dst]) - float(z["f64_iou"][b, t, src])))
        worst_pool = max(worst_pool, float(np.abs(got["pooled"][b, t, src].astype(np.float64) - z["f64_pooled"][b, t, src]).max()))
    print(f"max |kernel - f64|: IoU {worst_iou:.3e}, pooled {worst_pool:.3e}; tolerance {tol:.3e} "
          f"(reference f32: IoU {float(z['ref_f32_gap']):.3e}, pooled {float(z['ref_f32_pooled_gap']):.3e})")
    assert worst_iou <= tol
    assert worst_pool <= tol
    dead = z["ref_npts"] == 0
    assert (got["pooled"][dead] == 0).all()


def test_two_runs_are_bit_identical(z, dev, module, got):
    again = run(z, dev, module)
    for k in ("boxes", "scores", "labels", "counts", "npts", "pooled"):
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), k


def test_module_returns_lazy_detections_with_golden_entropy(z, dev, module):
    from al3d.models.bbox_heads import LazyDetections
    i = inputs(z, dev)
    done = torch.cuda.Event()
    done.record()
    meta = [dict(token=f"f{b}") for b in range(4)]
    preds = LazyDetections(i["boxes"], i["scores"], i["labels"], i["counts"], done, meta)
    with torch.no_grad():
        out = module(dict(preds=preds, points=i["points"], point_offsets=i["offsets"], middle=None), return_loss=False)
    assert isinstance(out, LazyDetections) and len(out) == 4
    ent = out.frame_entropy().cpu().numpy()
    tol = 4 * float(z["ref_f32_gap"])
    for b in range(4):
        p = np.array([z["f64_iou"][b_, t, src] for b_, t, src, _ in survivors(z) if b_ == b])
        want = EN.frame_entropy(p)
        if p.size == 0:
            assert np.isnan(ent[b])
            continue
        slope = np.abs(np.log((1 - p) / p)).max()
        assert abs(float(ent[b]) - want) <= slope * tol + 2e-6 * abs(want), (b, ent[b], want)
    # the other readers work on it unchanged
    w = torch.ones(10, device=dev)
    assert out.frame_weighted_entropy(w).shape == (4,)
    assert [int(d["scores"].shape[0]) for d in out] == z["ref_out_counts"].sum(axis=1).tolist()
    assert out[0]["metadata"] == meta[0] and out[0]["box3d_lidar"].shape[1] == 9 and out[0]["label_preds"].dtype == torch.int64
    refs = (i["boxes"][0, 0, :2, :].contiguous(), torch.zeros(2, dtype=torch.int32, device=dev),
            torch.ones(2, device=dev), torch.tensor([0, 2, 2, 2, 2], dtype=torch.int32, device=dev))
    assert out.match(refs, ncls=10)["match_ref"].shape == (4, 2, 8)


def test_list_and_batch_index_inputs_equal_the_raw_path(z, dev, module, got):
    i = inputs(z, dev)
    lists = []
    for b in range(4):
        sel = [(t, s) for t in range(2) for s in range(int(z["counts"][b, t]))]
        idx = torch.tensor([t * 8 + s for t, s in sel], dtype=torch.long, device=dev)
        lists.append(dict(box3d_lidar=i["boxes"][b].reshape(16, 9)[idx], scores=i["scores"][b].reshape(16)[idx],
                          label_preds=i["labels"][b].reshape(16)[idx].long(), metadata=dict(token=f"f{b}")))
    # the reference's points: [P, 1 + F] with the batch index first; frames interleaved on purpose
    off = z["offsets"]
    bidx = np.concatenate([np.full(int(off[b + 1] - off[b]), b, np.float32) for b in range(4)])
    perm = np.random.default_rng(0).permutation(len(bidx))       # max and count do not depend on the points' order
    pts = torch.from_numpy(np.concatenate([bidx[:, None], z["points"]], 1)[perm]).to(dev)
    with torch.no_grad():
        out = module(dict(preds=lists, points=pts, middle=None), return_loss=False)
    assert isinstance(out, list) and len(out) == 4
    for b in range(4):
        want_s = np.concatenate([got["scores"][b, t, :got["counts"][b, t]] for t in range(2)])
        want_b = np.concatenate([got["boxes"][b, t, :got["counts"][b, t]] for t in range(2)])
        assert np.array_equal(out[b]["scores"].cpu().numpy().view(np.int32), want_s.view(np.int32))
        assert np.array_equal(out[b]["box3d_lidar"].cpu().numpy().view(np.int32), want_b.view(np.int32))
        assert out[b]["metadata"] == dict(token=f"f{b}")


@pytest.mark.parametrize("case", ["descending", "beyond", "negative"])
def test_bad_point_offsets_raise_and_write_nothing(z, dev, module, case):
    from al3d import selector_ops as ops
    from al3d.lib import Al3dError
    i = inputs(z, dev)
    off = z["offsets"].copy()
    if case == "descending":
        off[2] = off[1] - 1
    elif case == "beyond":
        off[4] += 1
    else:
        off[0] = -1
    out = dict(boxes=torch.full_like(i["boxes"], 7.0), scores=torch.full((4, 2, 8), 7.0, device=dev),
               labels=torch.full_like(i["labels"], 7), counts=torch.full_like(i["counts"], 7))
    with pytest.raises(Al3dError, match="point_offsets"):
        ops.estimate_boxes(i["boxes"], i["labels"], i["counts"], i["points"], torch.from_numpy(off).to(dev),
                           module.packed_weights(dev), 10, out=out)
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in out.values())


def test_bad_label_raises_and_writes_nothing(z, dev, module):
    from al3d import selector_ops as ops
    from al3d.lib import Al3dError
    i = inputs(z, dev)
    i["labels"][0, 1, 2] = 10
    out = dict(boxes=torch.full_like(i["boxes"], 7.0), scores=torch.full((4, 2, 8), 7.0, device=dev),
               labels=torch.full_like(i["labels"], 7), counts=torch.full_like(i["counts"], 7))
    with pytest.raises(Al3dError, match="label"):
        ops.estimate_boxes(i["boxes"], i["labels"], i["counts"], i["points"], i["offsets"], module.packed_weights(dev), 10,
                           out=out)
    assert all(bool((v == 7).all()) for v in out.values())


def test_box_table_above_the_cap_raises_and_writes_nothing(z, dev, module):
    from al3d import selector_ops as ops
    from al3d.lib import Al3dError
    post = ops.EST_MAX_BOXES // 2 + 1                       # nt * post = 1026 > 1024
    boxes = torch.zeros((1, 2, post, 9), device=dev)
    out = dict(boxes=torch.full_like(boxes, 7.0), scores=torch.full((1, 2, post), 7.0, device=dev),
               labels=torch.full((1, 2, post), 7, dtype=torch.int32, device=dev),
               counts=torch.full((1, 2), 7, dtype=torch.int32, device=dev))
    with pytest.raises(Al3dError, match="at most 1024"):
        ops.estimate_boxes(boxes, torch.zeros((1, 2, post), dtype=torch.int32, device=dev),
                           torch.zeros((1, 2), dtype=torch.int32, device=dev), torch.zeros((4, 5), device=dev),
                           torch.tensor([0, 4], device=dev), module.packed_weights(dev), 10, out=out)
    assert all(bool((v == 7).all()) for v in out.values())


def _child(env):
    if _faulted:
        pytest.fail(f"not started: an earlier child ended with {_faulted[0]}", pytrace=False)
    full = {k: v for k, v in os.environ.items() if k != "AL3D_PIPELINE"}
    full.update(env)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "estimator_sweep_worker.py")]
    try:
        r = subprocess.run(cmd, env=full, timeout=CHILD_LIMIT_S, capture_output=True, text=True, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _faulted.append(f"time limit of {CHILD_LIMIT_S} s")
        pytest.fail(f"{env}: the child ran into its time limit", pytrace=False)
    if r.returncode < 0 or r.returncode in FAULT_CODES:
        _faulted.append(f"exit status {r.returncode}")
        pytest.fail(f"{env}: the child ended with status {r.returncode}\n{r.stderr[-4000:]}", pytrace=False)
    assert r.returncode == 0, r.stderr[-6000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_sweep_through_with_estimator_pipelined_equals_serial():
    """A tiny synthetic pool through ``WithEstimator``: the default pipelined sweep and ``AL3D_PIPELINE=0`` give the same
    entropies bit for bit, and they differ from the un-rescored sweep's."""
    piped = _child({})
    serial = _child({"AL3D_PIPELINE": "0"})
    assert piped["pipeline"] == "ahead" and serial["pipeline"] is None
    assert piped["rescored"] == serial["rescored"]
    assert piped["plain"] == serial["plain"]
    assert piped["boxes_frame0"] > 0
    ent = np.array(piped["rescored"], dtype=np.int32).view(np.float32)
    assert np.isfinite(ent).all()
    assert piped["rescored"][0] != piped["plain"][0] and piped["rescored"] != piped["plain"]
