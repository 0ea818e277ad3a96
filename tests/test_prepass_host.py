"""CPU suite for the PPAL / CALD pre-passes: the closing formulas of selectors/prepass.py against the golden written by
tools/gen_golden_prepass.py (the reference's own ``accumulate`` for the matching; restatements of ppal_unc.py:69-98 and
cald_ent.py:73-164 with the reference's numpy / scipy / torch calls for the formulas, on synthetic frames and on a slice
of 200 frames of the reference's recorded ``dict_p_iou.pkl``), the three file writers through the selectors' readers,
and ``CaldSelector``'s unchanged default path."""
import json
import os
import pickle

import numpy as np
import pytest

import prepass_numpy as PN

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "prepass_match.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def rec(z):
    """The recorded slice as the per-frame arrays the matching kernel would hand back."""
    return PN.frame_arrays(z["rec_frame"], z["rec_cls"], z["rec_score"], z["rec_iou"], z["rec_ref_score"],
                           int(z["rec_num_frames"]), 10)


def test_restatement_equals_the_reference_accumulate(z):
    """tests/prepass_numpy.py::match_frames (the expected values of the GPU edge cases) on the golden's inputs: every integer
    output equal to what the reference's accumulate produced, the float ones to float64 rounding."""
    got = PN.match_frames(z["boxes"], z["scores"], z["labels"], z["counts"], z["ref_boxes"], z["ref_labels"],
                          z["ref_scores"], z["ref_off"], 10, float(z["dist_th"]))
    assert np.array_equal(got["match_ref"], z["match_ref"]) and np.array_equal(got["cls_count"], z["cls_count"])
    assert (z["match_ref"] >= 0).sum() == z["cls_count"].sum() > 60
    np.testing.assert_allclose(got["match_iou"], z["match_iou"], rtol=1e-15, atol=0)
    np.testing.assert_allclose(got["cls_quality"], z["cls_quality"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(got["cls_cons"], z["cls_cons"], rtol=0, atol=1e-15)


def _weights(names, vals):
    return dict(zip([str(n) for n in names], vals.tolist()))


def test_ppal_class_weights_synthetic(z):
    from al3d.selectors.prepass import ppal_class_weights
    got = ppal_class_weights(z["cls_count"], z["cls_quality"], z["syn_labelled"].tolist(), z["names"].tolist())
    want = _weights(z["syn_weight_names"], z["syn_weight_vals"])
    assert set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k


@pytest.mark.parametrize("which", ["ppal", "all"])
def test_ppal_class_weights_recorded_slice(z, rec, which):
    """``ppal``: twelve labelled frames, six classes have no match among them and are absent from the dict."""
    from al3d.selectors.prepass import ppal_class_weights
    cnt, qual, _ = rec
    lab = z["rec_ppal_labelled" if which == "ppal" else "rec_cald_labelled"].tolist()
    want = _weights(z["rec_weight_names" if which == "ppal" else "rec_weight_all_names"],
                    z["rec_weight_vals" if which == "ppal" else "rec_weight_all_vals"])
    got = ppal_class_weights(cnt, qual, lab, z["names"].tolist())
    assert set(got) == set(want) and (which == "all" or len(got) < 10)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    assert all(isinstance(v, float) for v in got.values())


def test_cald_rankings_recorded_slice(z, rec):
    from al3d.selectors.prepass import cald_rankings
    cnt, _, cons = rec
    order, jsdiv = cald_rankings(cons, cnt, z["rec_cald_labelled"].tolist())
    assert order == z["rec_sorted"].tolist()                        # every frame, none left out
    # the 60 frames without a match stay at 1.0 and keep their dataset order behind the others (stable sort)
    frame_cons = z["rec_consistency"]
    tail = [i for i in order if frame_cons[i] == 1.0]
    assert len(tail) >= 60 and tail == sorted(tail) and order[-len(tail):] == tail
    assert list(jsdiv.keys()) == z["rec_jsdiv_keys"].tolist()       # inserted in sorted order, matched frames only
    np.testing.assert_allclose(np.array(list(jsdiv.values())), z["rec_jsdiv_vals"], rtol=1e-12, atol=1e-12)
    assert not set(jsdiv) & {i for i in range(len(order)) if cnt[i].sum() == 0}


def test_cald_rankings_synthetic_and_float32_inputs(z):
    """The kernel hands back float32 consistencies: the order of the golden's frames (more than 1e-4 apart) survives."""
    from al3d.selectors.prepass import cald_rankings
    order, jsdiv = cald_rankings(z["cls_cons"].astype(np.float32), z["cls_count"], z["syn_cald_labelled"].tolist())
    assert order == z["syn_sorted"].tolist() and list(jsdiv.keys()) == z["syn_jsdiv_keys"].tolist()
    np.testing.assert_allclose(np.array(list(jsdiv.values())), z["syn_jsdiv_vals"], rtol=1e-12, atol=1e-12)


def test_cald_rankings_refuses_what_the_reference_cannot_compute(z):
    from al3d.selectors.prepass import cald_rankings
    with pytest.raises(ValueError):
        cald_rankings(z["cls_cons"], z["cls_count"], [])
    with pytest.raises(IndexError):
        cald_rankings(np.ones((2, 11)), np.zeros((2, 11), np.int32), [0])


def test_frame_refs_from_infos_and_batches():
    import torch
    from al3d.selectors.prepass import FrameRefs
    infos = [dict(gt_boxes=np.arange(18, dtype=np.float32).reshape(2, 9), gt_names=np.array(["car", "ignore"])),
             dict(gt_boxes=np.zeros((0, 9), np.float32), gt_names=np.array([], dtype="<U8")),
             dict(gt_boxes=np.ones((1, 9), np.float32), gt_names=np.array(["bus"]))]
    refs = FrameRefs.from_infos(infos, ["car", "bus"])
    assert len(refs) == 3 and refs.off.tolist() == [0, 2, 2, 3] and refs.labels.tolist() == [0, -1, 1]
    assert np.all(refs.scores == -1.0)
    rb, rl, rs, ro = refs.batch([2, 1, 0], torch.device("cpu"))
    assert ro.tolist() == [0, 1, 1, 3] and ro.dtype == torch.int32 and rl.tolist() == [1, 0, -1]
    assert rb.shape == (3, 9) and rb[1].tolist() == list(range(9))
    empty = FrameRefs.from_frames(2, {})
    assert empty.off.tolist() == [0, 0, 0] and empty.boxes.shape == (0, 9)


def _cald_case(tmp_path):
    from al3d import synthetic
    zc = np.load(os.path.join(GOLDEN, "cald_seeded.npz"), allow_pickle=False)
    infos, _ = synthetic.make_pool(int(zc["pool_scenes"]), seed=int(zc["pool_seed"]))
    ip, bp = str(tmp_path / "infos.pkl"), str(tmp_path / "buffer.json")
    pickle.dump(infos, open(ip, "wb"))
    open(bp, "w").write(str(zc["buffer_json"]))
    return zc, ip, bp


@pytest.mark.parametrize("ext", ["pkl", "json"])
def test_writers_round_trip_through_cald_selector(tmp_path, ext):
    """The files written by ``write_ranking`` / ``write_jsdiv`` replay to the reference's golden selection."""
    from al3d.selectors import build_selector
    from al3d.selectors.prepass import write_jsdiv, write_ranking
    zc, ip, bp = _cald_case(tmp_path)
    sp, jp = str(tmp_path / "out" / "sorted.json"), str(tmp_path / "out" / f"jsdiv.{ext}")
    write_ranking(sp, zc["sorted_idx"])                              # numpy integers in, a JSON list out
    jsdiv = dict(zip(zc["jsdiv_keys"].tolist(), zc["jsdiv_vals"].tolist()))
    write_jsdiv(jp, jsdiv)
    assert json.load(open(sp)) == zc["sorted_idx"].tolist()
    assert sorted(os.listdir(tmp_path / "out")) == sorted(["sorted.json", f"jsdiv.{ext}"])       # no temporary file stays
    sel = build_selector(dict(type="CaldSelector", budget=int(zc["budget"]), buffer_file=bp, infos_origin=ip,
                              buffer_path=sp, jsdiv_path=jp))
    assert sel._load_jsdiv() == jsdiv
    sel.select_samples(local_rank=0)
    assert sel.selected_index[sel.current_budget] == zc["selected"].tolist()


def test_class_weight_file_reads_like_ppal_selector(tmp_path, z):
    """``PPALSelector.buffer_pred`` reads its ``class_weight_file`` with ``json.load`` and looks every class of the head up
    by name (uncertainty_selectors.py:242-245); the sweep itself needs a GPU, so the same two steps are done here."""
    from al3d.selectors.prepass import write_class_weights
    want = _weights(z["rec_weight_all_names"], z["rec_weight_all_vals"])
    path = str(tmp_path / "diff_category_average.json")
    write_class_weights(path, {k: np.float64(v) for k, v in want.items()})
    with open(path, "r") as f:
        class_weight = json.load(f)
    assert [class_weight[c] for c in want] == list(want.values())


def test_cald_selector_default_is_the_replay(tmp_path):
    """Without ``prepass`` nothing is swept or written: the golden replay of tests/test_host_logic.py, with a detector that
    would fail if touched."""
    from al3d.selectors import build_selector
    zc, ip, bp = _cald_case(tmp_path)
    sp, jp = str(tmp_path / "sorted.json"), str(tmp_path / "jsdiv.pkl")
    json.dump(zc["sorted_idx"].tolist(), open(sp, "w"))
    pickle.dump(dict(zip(zc["jsdiv_keys"].tolist(), zc["jsdiv_vals"].tolist())), open(jp, "wb"))
    before = (open(sp, "rb").read(), open(jp, "rb").read())

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the replay must not touch the detector")

    sel = build_selector(dict(type="CaldSelector", budget=int(zc["budget"]), buffer_file=bp, infos_origin=ip,
                              buffer_path=sp, jsdiv_path=jp, detector=Untouchable(), dataloader=Untouchable()))
    assert sel.prepass is False
    sel.select_samples(local_rank=0)
    assert sel.selected_index[sel.current_budget] == zc["selected"].tolist()
    assert (open(sp, "rb").read(), open(jp, "rb").read()) == before
    with pytest.raises(ValueError):
        build_selector(dict(type="CaldSelector", budget=int(zc["budget"]), buffer_file=bp, infos_origin=ip,
                            buffer_path=sp, jsdiv_path=jp, prepass=True)).select_samples(local_rank=0)
