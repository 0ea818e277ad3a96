"""CPU suite: the batch of tests/sweep_batch_cases.py has the shape and the teeth tests/test_sweeps_batch_gpu.py relies on."""
import numpy as np

import sweep_batch_cases as S


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_the_batch_has_the_frames_it_promises(oracle):
    frames = S.build()
    k = S.kernel_arrays(frames)
    assert k["n_frames"] == 5 and k["total"] > 4096                          # the scan's workgroups end at 2048 and 4096
    rows = [int(k["file_off"][k["frame_first_file"][b + 1]] - k["file_off"][k["frame_first_file"][b]]) for b in range(5)]
    assert rows[0] > 0 and rows[1] == 0 and rows[2] > 0 and rows[3] > 0 and rows[4] == 0
    assert k["file_off"][k["frame_first_file"][4]] == k["total"]             # the last frame starts at the end of the input
    assert len(frames[3]["key"]) == 0 and all(len(s["points"]) for s in frames[3]["sweeps"])
    assert [s["has_xform"] for s in frames[0]["sweeps"]] == [True, False, True]
    for rule in (0, 1):
        for filtered in (False, True):
            n = [len(p) for p in S.reference(oracle, frames, rule, filtered)]
            assert n[0] > 1000 and n[1] == 0 and n[2] == 0 and n[3] > 1000 and n[4] == 0, (rule, filtered, n)


def test_rule_one_reference_is_the_elementwise_statement(oracle):
    frames = S.build()
    for f, ref in zip(frames, S.reference(oracle, frames, 1, False)):
        assert np.array_equal(_bits(ref), _bits(S.rule1_by_hand(f)))


def test_the_two_rules_differ_and_the_filter_is_strict(oracle):
    frames = S.build()
    r0, r1 = S.reference(oracle, frames, 0, False), S.reference(oracle, frames, 1, False)
    differ = 0
    for a, b in zip(r0, r1):
        assert a.shape == b.shape                                             # the rules keep the same points ...
        differ += int(np.any(_bits(a) != _bits(b), axis=1).sum())
    assert differ >= 100, differ                                              # ... at other float32 values
    pts, inside = S.boundary_points()
    assert len(pts) == 12 and inside.sum() == 6
    lo, hi = np.asarray(S.RANGE[:3], np.float32), np.asarray(S.RANGE[3:], np.float32)
    for rule in (0, 1):
        plain, filt = S.reference(oracle, frames, rule, False)[0], S.reference(oracle, frames, rule, True)[0]
        tagged = plain[plain[:, 3] >= S.TAG]
        assert np.array_equal(tagged[:, 3], S.TAG + np.arange(12, dtype=np.float32))
        for j, p in enumerate(tagged):                                       # the transformed value IS the bound, or one ulp inside
            d, which = j // 4, j % 4
            want = [lo[d], np.nextafter(lo[d], np.float32(np.inf)), hi[d], np.nextafter(hi[d], np.float32(-np.inf))][which]
            assert _bits(p[d:d + 1])[0] == _bits(np.array([want]))[0]
        kept = filt[filt[:, 3] >= S.TAG][:, 3] - S.TAG
        assert kept.astype(int).tolist() == np.flatnonzero(inside).tolist()
        assert np.isnan(plain[:, 0]).sum() == 1 and not np.isnan(filt).any()  # the NaN point: kept without the filter only
        assert len(filt) < len(plain) - 7
