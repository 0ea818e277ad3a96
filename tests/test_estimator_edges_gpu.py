"""GPU suite for the edges of csrc/estimator.hip that tests/golden/estimator.npz does not reach: hits in every frame, the
mid-loop queue drain at exactly EST_QCAP and at the threshold plus one, more than 64 boxes per task, more than 16 survivors
per (frame, task), a full box table, other box / point / class layouts, and NaN, inf, zero and negative values.  The inputs are
the generated cases of tests/estimator_cases.py (tests/test_estimator_cases_cpu.py checks that each reaches its path);
``selector_ops.estimate_boxes`` is called directly and compared with the float64 yardstick tests/estimator_numpy.py.  Kernel
output is compared with kernel output in two places only, both beside the yardstick comparison: two runs of one case, and
the clean against the dirty variants of the values family.

Exact: point counts, new counts, status, survivors and their order, the survivors' box bits and labels, zero pooled rows
where the yardstick has no point, zero outputs behind the new counts.  Numeric: 4 x the float32 torch evaluation's own
distance from float64 on the same case (tests/estimator_f32.py); the factor is the one tests/test_estimator_gpu.py uses.
Every numeric test prints its figures."""
import numpy as np
import pytest
import torch

import estimator_cases as EC
import estimator_f32 as E32

pytestmark = pytest.mark.gpu

_results = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def launch(name, dev):
    from al3d import selector_ops as ops
    c = EC.case(name)
    t = lambda k: torch.from_numpy(c[k]).to(dev)            # noqa: E731
    res = ops.estimate_boxes(t("boxes"), t("labels"), t("counts"), t("points"), t("offsets"),
                             E32.module(c["classes"]).packed_weights(dev), c["num_classes"], rot_col=c["rot_col"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def run(name, dev):
    """The case's first run, shared by the tests."""
    if name not in _results:
        _results[name] = launch(name, dev)
    return _results[name]


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name", EC.NAMES)
def test_counts_survivors_boxes_and_labels_exact(name, dev):
    c, y, got = EC.case(name), E32.yardstick(name), run(name, dev)
    B, nt, post, D = c["boxes"].shape
    assert int(got["status"][0]) == 0
    assert np.array_equal(got["npts"], y["npts"])           # the yardstick has 0 behind the counts
    assert np.array_equal(got["counts"], y["counts"])
    assert (got["pooled"][y["npts"] == 0] == 0).all()
    for b in range(B):
        for t in range(nt):
            keep = y["survivors"][b * nt + t]               # ascending slots: the compaction is stable
            n = len(keep)
            assert np.array_equal(got["boxes"][b, t, :n].view(np.int32), c["boxes"][b, t, keep].view(np.int32))
            assert np.array_equal(got["labels"][b, t, :n], c["labels"][b, t, keep])
            assert np.isfinite(got["scores"][b, t, :n]).all()
            # nothing is written behind the new count (the buffers start zeroed)
            assert not got["boxes"][b, t, n:].view(np.int32).any() and not got["scores"][b, t, n:].view(np.int32).any()
            assert not got["labels"][b, t, n:].any()


@pytest.mark.parametrize("name", EC.NAMES)
def test_ious_and_pooled_rows_within_four_float32_gaps(name, dev):
    c, y, got = EC.case(name), E32.yardstick(name), run(name, dev)
    nt = c["labels"].shape[1]
    e_iou = e_pooled = 0.0
    for b, t, i in y["owners"]:
        dst = y["survivors"][b * nt + t].index(i)
        e_iou = max(e_iou, abs(float(got["scores"][b, t, dst]) - float(y["iou"][b, t, i])))
        e_pooled = max(e_pooled, float(np.abs(got["pooled"][b, t, i].astype(np.float64) - y["pooled"][b, t, i]).max()))
    print(f"| {name} | {len(y['owners'])} | {e_iou:.3e} | {y['e32_iou']:.3e} | {e_iou / y['e32_iou']:.2f} | "
          f"{e_pooled:.3e} | {y['e32_pooled']:.3e} | {e_pooled / y['e32_pooled']:.2f} |")
    assert e_iou <= 4 * y["e32_iou"]
    assert e_pooled <= 4 * y["e32_pooled"]


@pytest.mark.parametrize("name", ["A", "B1", "C"])
def test_two_runs_are_bit_identical(name, dev):
    first, again = run(name, dev), launch(name, dev)
    for k in ("boxes", "scores", "labels", "counts", "npts", "pooled"):
        assert np.array_equal(bits(first[k]), bits(again[k])), k


@pytest.mark.parametrize("name", ["F_dirty1", "F_dirty2"])
def test_dirty_boxes_and_points_change_nothing_else(name, dev):
    """Every slot that is ordinary in both runs: the same count, pooled row and score bits, at the same compacted
    position -- the dirty boxes sit in task 0's last slots and drop out, as the clean run's far boxes do."""
    c = EC.case(name)
    clean, dirty = run("F_clean", dev), run(name, dev)
    assert np.array_equal(clean["counts"], dirty["counts"])
    for k in ("scores", "labels", "boxes"):                 # compacted: the survivors are ordinary slots in both
        assert np.array_equal(bits(clean[k]), bits(dirty[k])), k
    ordinary = np.ones(16, dtype=bool)
    ordinary[c["reach"]["dirty_slots"]] = False
    for k in ("npts", "pooled"):                            # per input slot
        a, d = clean[k].reshape(16, -1)[ordinary], dirty[k].reshape(16, -1)[ordinary]
        assert np.array_equal(bits(a), bits(d)), k
    assert (dirty["npts"].reshape(16)[~ordinary] == 0).all() and (dirty["pooled"].reshape(16, 128)[~ordinary] == 0).all()
