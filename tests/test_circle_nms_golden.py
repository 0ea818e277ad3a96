"""CPU suite: ``transfusion_head.circle_nms`` against the reference's own function
(bevfusion/mmdet3d/core/post_processing/box3d_nms.py:180-219), run as plain Python by oracle/gen_golden_bevfusion_models.py:
tests/golden/bevfusion_circle_nms.npz holds the inputs and the kept indices of n in {0, 1, 2, 200}, exactly equal scores,
pairs whose float32 squared distance is one ulp under, at and one ulp over float32(0.175) and float32(0.7), and 120
isolated points that ``post_max_size`` cuts.  The same lists, in the same order."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bevfusion_circle_nms.npz")
NAMES = [str(n) for n in np.load(GOLD)["names"]]


@pytest.mark.parametrize("name", NAMES)
def test_circle_nms_keeps_what_the_reference_keeps(name):
    from al3d.models.transfusion_head import circle_nms
    z = np.load(GOLD)
    dets, thresh, post = z[f"{name}.dets"], float(z[f"{name}.thresh"][0]), int(z[f"{name}.post_max_size"][0])
    assert dets.dtype == np.float32 and dets.shape[1] == 3
    want = z[f"{name}.keep"].tolist()
    assert circle_nms(dets, thresh, post) == want
    if post == 83:
        assert circle_nms(dets, thresh) == want                        # the default cut


def test_golden_holds_the_cases_it_is_for():
    z = np.load(GOLD)
    assert sorted(len(z[f"{n}.dets"]) for n in NAMES if n.startswith("n")) == [0, 1, 2, 2, 200, 200]
    assert len(np.unique(z["equal_scores_all.dets"][:, 2])) == 1 and len(np.unique(z["equal_scores_groups.dets"][:, 2])) == 9
    for thresh in (0.175, 0.7):
        t32 = np.float32(thresh)
        for rel, want, kept in (("under", np.nextafter(t32, np.float32(0)), [0, 2]), ("at", t32, [0, 2]),
                                ("over", np.nextafter(t32, np.float32(1)), [0, 1, 2])):
            d = z[f"pair_{rel}_{thresh}.dets"]
            assert (d[0, 0] - d[1, 0]) ** 2 + (d[0, 1] - d[1, 1]) ** 2 == want      # in float32, as the function evaluates it
            assert z[f"pair_{rel}_{thresh}.keep"].tolist() == kept
    assert len(z["isolated120_cut_at_83.keep"]) == 83 and len(z["isolated120_cut_at_83.dets"]) == 120
    assert len(z["isolated120_cut_at_10.keep"]) == 10
    assert 0 < len(z["n200_r0175.keep"]) < 83 and 0 < len(z["n200_r07.keep"]) < 83         # suppression, not the cut
