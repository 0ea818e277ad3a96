"""GPU suite: al3d_merge_sweeps_batch_range_f32 on raw arrays (no files, no loader) against the per-frame references of
tests/sweep_batch_cases.py, bit for bit: both transform rules, with and without the range filter, frames without rows in
the middle and at the end of the batch, a frame that loses every point, and points exactly on the filter's bounds."""
import ctypes

import numpy as np
import pytest
import torch

import sweep_batch_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0x7FC12345                    # a NaN pattern no kernel writes


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def batch():
    frames = S.build()
    k = S.kernel_arrays(frames)
    dev = {n: torch.from_numpy(np.ascontiguousarray(k[n])).to(DEV)
           for n in ("raw", "file_off", "xform", "has_xform", "time_lag", "is_key", "frame_first_file")}
    return frames, k, dev


def merge(k, dev, rule, filtered):
    from al3d import lib
    total, B = k["total"], k["n_frames"]
    out = torch.full((total, 5), FILL, dtype=torch.int32, device=DEV)
    frame_off = torch.full((B + 1,), -1, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.load().al3d_merge_sweeps_workspace_bytes(total), dtype=torch.uint8, device=DEV)
    rg = (ctypes.c_float * 6)(*S.RANGE) if filtered else None
    lib.call("al3d_merge_sweeps_batch_range_f32", dev["raw"].data_ptr(), dev["file_off"].data_ptr(), k["nfiles"], total,
             dev["xform"].data_ptr(), dev["has_xform"].data_ptr(), dev["time_lag"].data_ptr(), dev["is_key"].data_ptr(),
             dev["frame_first_file"].data_ptr(), B, S.MIN_DISTANCE, rule, rg, out.data_ptr(), frame_off.data_ptr(),
             ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), frame_off.cpu().numpy()


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("rule", [0, 1])
def test_batched_merge_equals_the_per_frame_references(oracle, batch, rule, filtered):
    frames, k, dev = batch
    want = S.reference(oracle, frames, rule, filtered)
    out, frame_off = merge(k, dev, rule, filtered)
    assert frame_off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert frame_off[1] == frame_off[3] and frame_off[4] == frame_off[5]      # the frames without a point
    for b, w in enumerate(want):
        assert np.array_equal(out[frame_off[b]:frame_off[b + 1]], _bits(w)), b
    assert np.all(out[frame_off[-1]:] == FILL)                               # nothing written behind the last point
    nan_rows = int(np.isnan(out[:frame_off[-1]].view(np.float32)[:, 0]).sum())
    assert nan_rows == (0 if filtered else 1)


def test_the_rule_switch_reaches_the_kernel(batch):
    _, k, dev = batch
    a, off_a = merge(k, dev, 0, False)
    b, off_b = merge(k, dev, 1, False)
    assert np.array_equal(off_a, off_b)
    assert int(np.any(a[:off_a[-1]] != b[:off_b[-1]], axis=1).sum()) >= 100
