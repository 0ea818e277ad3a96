"""GPU suite: ``al3d_head_decode_nms`` (csrc/head_nms.hip) on the planted cases of tests/anchorhead_cases.py against the
float64 yardstick tests/head_fp64.py -- kept anchors and their order exactly, labels, scores to 2e-7, boxes to 1e-6 relative,
angles to 2e-6 modulo 2 pi, counts, and nothing written past counts.  The cases stay off every threshold by the band measured
in anchorhead_cases (tests/test_anchorhead_fp64_cpu.py checks that on the CPU); tight_bounds holds both role assignments of
each pair (the second half of its samples)."""
import pytest

import anchorhead_cases as AC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family,placement", AC.CASES)
def test_anchor_head_equals_the_float64_yardstick(family, placement):
    case, ref, _ = AC.make(family, placement)
    got = AC.run_library(case)
    kept = sum(len(r["anchors"]) for row in ref for r in row)
    print(family, placement, "problems", len(ref) * len(ref[0]), "detections", kept)
    assert kept > 0
    AC.compare(case, ref, got)
