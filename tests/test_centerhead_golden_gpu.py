"""GPU: the reference coder's golden inputs (tests/golden/centerhead.npz) through ``al3d_center_decode_nms_f32``: the
survivors of ``CenterPointBBoxCoder.decode`` and the keeps of ``circle_nms`` come out equal, in the same order; and the
command line runs the CenterHead example config.  Bounds: those of tests/test_centerhead_golden.py with the device's
2-ulp expf / atan2f and sigmoid (4u on the score)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "centerhead.npz"))
U = 2.0 ** -24


def _run(name, transposed, radius, post):
    from al3d import detector_ops as D
    ncls, K, has_vel, has_reg = (int(v) for v in G[f"{name}.cfg"][:4])
    thr = float(G[f"{name}.cfg"][4])
    parts, chan, o = [], {}, 0
    for key, on in (("heat", True), ("reg", has_reg), ("height", True), ("dim", True), ("rot", True), ("vel", has_vel)):
        chan[key] = o if on else -1
        if on:
            parts.append(G[f"{name}.{key}"])
            o += parts[-1].shape[1]
    h = np.concatenate(parts, axis=1).transpose(0, 3, 2, 1) if transposed else np.concatenate(parts, axis=1).transpose(0, 2, 3, 1)
    geom = G["geom"]
    out = D.center_decode_nms(
        torch.from_numpy(np.ascontiguousarray(h)).cuda(), [ncls], [[chan[k] for k in ("heat", "reg", "height", "dim", "rot", "vel")]],
        swapped=transposed, max_num=K, norm_bbox=True, out_size_factor=geom[0], voxel_size=geom[1:3], pc_range=geom[3:5],
        coder_score_threshold=thr, post_center_range=G["post_center_range"], nms_type="circle", nms_scale=[[1.0] * ncls],
        min_radius=[radius], score_threshold=0.0, nms_thr=0.0, pre_max_size=1000, post_max_size=post,
        post_center_limit_range=None, merge=False)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out], (9 if has_vel else 7)


def _check(got, width, i, want_boxes, want_scores, want_labels):
    boxes, scores, labels, counts = got
    n = len(want_scores)
    assert int(counts[i, 0]) == n
    assert np.array_equal(labels[i, 0, :n], want_labels.astype(np.int32))
    assert np.all(np.abs(scores[i, 0, :n].astype(np.float64) - want_scores) <= 4 * U), "survivors / order"
    err = np.abs(boxes[i, 0, :n, :width].astype(np.float64) - want_boxes)
    assert np.all(err[:, :2] <= 5 * U * 16) and np.all(err[:, 2] == 0) and np.all(err[:, 7:] == 0)
    assert np.all(err[:, 3:6] <= 4 * U * want_boxes[:, 3:6]) and np.all(err[:, 6] <= 3 * 2.0 ** -22)
    assert np.all(boxes[i, 0, :n, width:] == 0)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("name", [str(n) for n in G["case_names"]])
def test_golden_through_the_kernel(name, transposed):
    K, radius, post = int(G[f"{name}.cfg"][1]), float(G[f"{name}.cfg"][5]), int(G[f"{name}.cfg"][6])
    survivors, width = _run(name, transposed, -1.0, K)         # a negative radius suppresses nothing: decode's survivors
    kept, _ = _run(name, transposed, radius, post)
    for i in range(2):
        wb, ws, wl = (G[f"{name}.{i}.{k}"].astype(np.float64) for k in ("bboxes", "scores", "labels"))
        _check(survivors, width, i, wb, ws, wl)
        keep = G[f"{name}.{i}.circle_keep"]
        _check(kept, width, i, wb[keep], ws[keep], wl[keep])


def test_cli_centerhead_config(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "active_select.py"), "--config",
           os.path.join(ROOT, "examples", "active", "bevfusion_lidar_centerhead_entropy.py"), "--budget", "20", "--pred",
           "--synthetic-scenes", "2", "--batch", "4"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for _ in range(2):                       # bootstrap the empty buffer, then sweep + select
        r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    out = json.load(open(tmp_path / "data" / "buffers" / "bevfusion_lidar_centerhead_entropy.json"))
    assert list(out) == ["0", "20"] and len(out["20"]) >= 1 and len(set(out["20"])) == len(out["20"])
