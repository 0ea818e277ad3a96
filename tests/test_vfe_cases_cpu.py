"""CPU suite: the cases of tests/vfe_cases.py meet the conditions they were chosen for, and the checker of
tests/vfe_fp64.py is sound.  These are conditions on the cases and the checker, not measurements of the kernel
(tests/test_vfe_edges_gpu.py runs the HIP code on the same cases)."""
import numpy as np
import pytest

import vfe_cases as C
import vfe_fp64 as V


def _all_shapes():
    out = [(C.SIZES_T, F, wd, f, 0) for F, wd, f in C.SIZES]
    out += [(T, 5, T == 64, f, 0) for T, f in C.COUNT_RUNS]
    out += [args for args, _ in C.LDS_SHAPES]
    return out


def test_sizes_cover_what_the_issue_lists():
    assert {(F, wd) for F, wd, _ in C.SIZES} == {(F, wd) for F in (3, 4, 5, 10) for wd in (0, 1)}
    assert sorted(map(tuple, C.ALL_FILTERS)) == sorted({tuple(f) for _, _, f in C.SIZES})
    k1 = {C.launch_shape(C.SIZES_T, F, wd, f)[3] for F, wd, f in C.SIZES}
    assert k1 == {6, 7, 8, 9, 13, 14}
    for flt in ([96], [96, 96]):                                  # 48 units: with zero-padded weight rows and without
        pads = {C.launch_shape(C.SIZES_T, F, wd, f)[4] > C.launch_shape(C.SIZES_T, F, wd, f)[3]
                for F, wd, f in C.SIZES if f == flt}
        assert True in pads
    assert any(C.launch_shape(C.SIZES_T, F, wd, f)[3] == C.launch_shape(C.SIZES_T, F, wd, f)[4] for F, wd, f in C.SIZES)


def test_lds_cases_reach_every_launch_shape():
    want = [(16, 8), (2, 8), (1, 8), (1, 4), (1, 2), (1, 1)]
    got = []
    for args, shape in C.LDS_SHAPES:
        v, wpb, nbytes, _, _ = C.launch_shape(*args)
        assert (v, wpb) == shape, (args, v, wpb)
        got.append((v, wpb))
        print(f"{args}: V {v} wpb {wpb} {nbytes} bytes")
    assert got == want
    by_args = {(a[0], a[1], a[2], tuple(a[3])): C.launch_shape(*a)[2] for a, _ in C.LDS_SHAPES}
    assert by_args[(10, 5, 0, (128, 128))] == 152832
    assert by_args[(64, 5, 0, (32, 128))] == 125760
    assert by_args[(64, 10, 1, (128, 128))] == 143904
    assert C.launch_shape(64, 10, 1, [128, 128])[3:] == (14, 16)
    # the step in front of each shape does not fit: the ladder really is walked down to it
    assert C.launch_shape(20, 5, 0, [128, 128])[1] == 4 and C.launch_shape(10, 5, 0, [128, 128])[1] == 8


def test_every_case_fits_the_lds():
    for args in _all_shapes():
        assert C.launch_shape(*args)[2] <= C.LDS_LIMIT, args
    assert C.launch_shape(5, 5, 0, [64], 5)[0] == 5               # a stated V is kept where it fits
    assert C.launch_shape(10, 5, 0, [32, 128], 16)[0] == 2        # and shrunk where it does not
    # voxels_per_wave = 16: kept at 16 (once 3,840 bytes under the limit), and shrunk to a V above anything the default asks
    assert [C.launch_shape(*a, 16)[:2] for a in C.VPW16_RUNS] == [(16, 8), (16, 8), (8, 8)]
    assert C.launch_shape(*C.VPW16_RUNS[1], 16)[2] == 160000


def _f32_level(c):
    """e32 of a case and the first-order bound B it must stay under: a float32 evaluation IS what B bounds."""
    ref, absum = V.vfe_net(c["vox"], c["num"], c["layers"], c["wd"])
    assert (absum > 0).all() and np.isfinite(ref).all()
    errs = {o: V.err(V.vfe_net_f32(c["vox"], c["num"], c["layers"], c["wd"], o), ref, absum) for o in V.ORDERS}
    e32 = V.e32(c["vox"], c["num"], c["layers"], c["wd"], ref, absum)
    assert e32 == max(errs.values())
    B = V.bound(c["T"], C.widths(c["layers"]))
    return e32, B, errs


@pytest.mark.parametrize("F,wd,filters", C.SIZES)
def test_f32_evaluation_is_float32_level_on_sizes(F, wd, filters):
    e32, B, errs = _f32_level(C.size_case(F, wd, filters))
    print(f"F {F} wd {wd} {filters}: e32 = {e32:.3e} ({errs}), B = {B:.3e}")
    assert 0 < e32 <= B


def test_f32_evaluation_is_float32_level_on_counts_and_lds_cases():
    cases = [C.count_case(T, f) for T, f in C.COUNT_RUNS]
    cases += [C.lds_case(*args[:4], 70) for args, _ in C.LDS_SHAPES]
    cases += [C.vfe1_pad_fixture(), C.vfe2_pad_fixture()]
    for c in cases:
        e32, B, _ = _f32_level(c)
        print(f"T {c['T']} F {c['F']} {c['filters']}: e32 = {e32:.3e}, B = {B:.3e}")
        assert 0 < e32 <= B


def test_f32_evaluation_rounds_every_operation():
    """float32 output, the three orders differ among themselves (they are three roundings, not one), and a count of 0
    gives the zero row."""
    c = C.size_case(5, 1, [32, 128])
    outs = [V.vfe_net_f32(c["vox"], c["num"], c["layers"], c["wd"], o) for o in V.ORDERS]
    assert all(o.dtype == np.float32 and o.shape == (C.SIZES_M, 128) for o in outs)
    assert not np.array_equal(outs[0], outs[1])
    assert c["num"][0] == 0 and not any(o[0].any() for o in outs)


def test_counts_cover_every_chunk_edge():
    c = C.count_case(17, [64])
    assert sorted(c["num"].tolist()) == sorted(list(range(18)) * 4) and c["vox"].shape == (72, 17, 5)
    assert c["num"].tolist() != sorted(c["num"].tolist())
    c = C.count_case(64, [32, 128])
    assert sorted(set(c["num"].tolist())) == [0, 1, 63, 64] and c["wd"]


def test_vfe1_fixture_tells_the_readings_apart():
    c = C.vfe1_pad_fixture()
    h, real = C.hidden_rows(c, 0)
    assert (c["num"] == 1).all()
    assert (h[:, 1] > h[:, 0]).mean() > 0.5                      # a padded slot wins for most of vfe1's units
    ref, absum = V.vfe_net(c["vox"], c["num"], c["layers"], False)
    wrong, _ = V.vfe_net(c["vox"], c["num"], c["layers"], False, pad_in_max1=False)
    B = V.bound(c["T"], C.widths(c["layers"]))
    assert (np.abs(wrong - ref) > 10 * B * absum).any(1).all()   # in every voxel


def test_vfe2_fixture_tells_the_readings_apart():
    c = C.vfe2_pad_fixture()
    h, real = C.hidden_rows(c, 1)
    w2, s2, b2 = c["layers"][1]
    assert (w2 < 0).all() and (s2 == 1).all() and (b2 >= 1).all()
    part = c["num"] < c["T"]
    assert part.sum() >= 50 and (~part).sum() == 4
    for m in np.flatnonzero(part):
        n = c["num"][m]
        assert np.array_equal(h[m, n], b2)                       # a padded slot holds relu(b2) ...
        assert (h[m, :n] <= b2).all() and (h[m, :n] < b2).mean() > 0.9      # ... and the real rows lie below it
    assert (h[real] > 0).mean() > 0.75                           # and are alive: no row of zeros stands in for them
    ref, absum = V.vfe_net(c["vox"], c["num"], c["layers"], False)
    wrong, _ = V.vfe_net(c["vox"], c["num"], c["layers"], False, pad_in_max2=False)
    B = V.bound(c["T"], C.widths(c["layers"]))
    moved = (np.abs(wrong - ref) > 10 * B * absum).any(1)
    assert moved[part].all() and not moved[~part].any()
    assert np.array_equal(wrong[~part], ref[~part])
    # pad_in_max2 is no other name for pad_in_max1, and means nothing with one VFE layer
    w1, _ = V.vfe_net(c["vox"], c["num"], c["layers"], False, pad_in_max1=False)
    assert not np.array_equal(w1, wrong)
    one = C.size_case(4, 0, [64])
    assert np.array_equal(V.vfe_net(one["vox"], one["num"], one["layers"], False, pad_in_max2=False)[0],
                          V.vfe_net(one["vox"], one["num"], one["layers"], False)[0])


@pytest.mark.parametrize("filters", C.NAN_FILTERS)
def test_nan_rule_restatement(filters):
    """nan_rule changes nothing on finite input; on the NaN cases the plain reference gives NaN in exactly the affected
    voxels, the rule gives finite rows there with a finite positive absum, and the other voxels keep their values.  A NaN
    in a coordinate leaves the voxel as if vfe1 had given 0 everywhere."""
    for wd in (False, True):
        c, clean, hit = C.nan_case(filters, wd)
        a = V.vfe_net(clean, c["num"], c["layers"], wd)
        b = V.vfe_net(clean, c["num"], c["layers"], wd, nan_rule=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        plain, _ = V.vfe_net(c["vox"], c["num"], c["layers"], wd)
        rule, absum = V.vfe_net(c["vox"], c["num"], c["layers"], wd, nan_rule=True)
        assert np.flatnonzero(np.isnan(plain).any(1)).tolist() == hit
        assert np.isfinite(rule).all() and np.isfinite(absum).all() and (absum > 0).all()
        keep = np.setdiff1d(np.arange(len(c["num"])), hit)
        assert np.array_equal(rule[keep], a[0][keep])
        assert not np.array_equal(rule[5], a[0][5])              # the killed slot's row is missed
        # NaN mean: every vfe1 row is 0, so the rest of the net sees zeros in the real slots
        x = np.zeros((1, c["T"], c["layers"][1][0].shape[1]))
        for w, s, sh in c["layers"][1:]:
            y = np.maximum(x @ w.T * s + sh, 0.0)
            x = np.concatenate([y, np.repeat(y.max(1)[:, None, :], c["T"], 1)], -1)
        assert np.allclose(rule[20], y[0, 0], rtol=1e-12, atol=0) and np.allclose(rule[33], y[0, 0], rtol=1e-12, atol=0)
