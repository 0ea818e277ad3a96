"""CPU suite: detector_ops.dense_structure over the layers of the SECOND neck and head, under each arithmetic and every
AL3D_DENSE setting, and the DENSE_KINDS table.  The expected kinds are what pack_dense returned before its policy moved
behind dense_structure."""
import os
import re

import pytest

from al3d import detector_ops as D

# (cout, cin, ksize, stride, pad): A-D the 3x3 layers of the two blocks (C the stride-2 entry), E / F the deblocks (1x1
# conv, 2x2 transposed conv), G the fused head, N a narrow 3x3 the 16x16x32 fragment shape cannot take (Cin % 64 != 0)
A, B, C, Dl = (128, 256, 3, 1, 1), (128, 128, 3, 1, 1), (256, 128, 3, 2, 1), (256, 256, 3, 1, 1)
E, F, G, N = (256, 128, 1, 1, 0), (256, 256, "deconv"), (180, 512, 1, 1, 0), (128, 32, 3, 1, 1)
LAYERS = (A, B, Dl, N, C, E, F, G)
DENSE_VALUES = ("auto", "dma", "wino", "lds", "frag", "frag16", "stream", "bstream")


def _row(abd, n, c, e, f, g):
    return [abd] * 3 + [n, c, e, f, g]


# DENSE -> kinds of (A, B, D, N, C, E, F, G) under f16x3.  "stream": C has 72 steps, G 32 (>= 24: streamed weights), E 8
# (LDS-staged), F is the deconv (LDS-staged)
F16X3 = {
    "auto": _row("frag3x3", "frag3x3", "dma", "dma", "dma", "dma"),
    "dma": _row("frag3x3", "frag3x3", "dma", "dma", "dma", "dma"),
    "wino": _row("wino", "wino", "dma", "dma", "dma", "dma"),
    "lds": _row("f16x3", "f16x3", "f16x3", "f16x3", "f16x3", "f16x3"),
    "frag": _row("frag3x3", "frag3x3", "f16x3", "f16x3", "f16x3", "f16x3"),
    "frag16": _row("frag16", "frag3x3", "f16x3", "f16x3", "f16x3", "f16x3"),
    "stream": _row("frag3x3", "frag3x3", "bstream", "f16x3", "f16x3", "bstream"),
    "bstream": _row("frag3x3", "frag3x3", "bstream", "bstream", "bstream", "bstream"),
}
CASES = [("f16x3", dense, want) for dense, want in F16X3.items()] + \
        [(math, dense, [math] * 8) for math in ("bf16x6", "f32") for dense in DENSE_VALUES]


@pytest.fixture
def settings():
    saved = D.MATH, D.DENSE
    try:
        yield
    finally:
        D.MATH, D.DENSE = saved


@pytest.mark.parametrize("math,dense,want", CASES, ids=[f"{m}-{d}" for m, d, _ in CASES])
def test_neck_and_head_structures(settings, math, dense, want):
    D.MATH, D.DENSE = math, dense
    assert [D.dense_structure(*layer) for layer in LAYERS] == want


def test_an_unrecognised_dense_value_behaves_like_frag(settings):
    D.MATH, D.DENSE = "f16x3", "no-such-structure"
    assert [D.dense_structure(*layer) for layer in LAYERS] == F16X3["frag"]


@pytest.mark.parametrize("dense", DENSE_VALUES)
def test_without_geometry_f16x3_weights_stay_plain_planes(settings, dense):
    D.MATH, D.DENSE = "f16x3", dense
    assert [D.dense_structure(layer[0], layer[1]) for layer in LAYERS] == ["f16x3"] * 8
    assert [D.dense_structure(layer[0], layer[1], None) for layer in LAYERS] == ["f16x3"] * 8


def test_every_kind_is_described_once_with_its_capabilities():
    """kind -> (generic geometry, deconv, io bits, fused GAP), and entry points that the C header declares."""
    none, out, both = 0, D.IO_OUT_PAIR, D.IO_IN_PAIR | D.IO_OUT_PAIR
    want = {
        "f32": (True, True, none, None), "bf16x6": (True, True, none, None), "f16x3": (True, True, none, "entry"),
        "frag3x3": (False, False, out, None), "wino": (False, False, out, None), "frag16": (False, False, none, None),
        "bstream": (True, True, none, None), "dma": (True, True, both, "arg"),
    }
    assert {k: (r.generic, r.deconv is not None, r.io, r.gap) for k, r in D.DENSE_KINDS.items()} == want
    assert (D.IO_IN_PAIR, D.IO_OUT_PAIR) == (1, 2)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "al3d.h")).read()
    declared = set(re.findall(r"\b(al3d_\w+)\s*\(", header))
    names = [fn for r in D.DENSE_KINDS.values() for fn in (r.conv, r.deconv) if fn is not None]
    names += [fn + "_gap" for r in D.DENSE_KINDS.values() if r.gap == "entry" for fn in (r.conv, r.deconv)]
    assert len(set(names)) == len(names) == 15 and set(names) <= declared
    assert all(callable(r.pack) for r in D.DENSE_KINDS.values())


def test_gap_fusable_reads_the_table():
    """True exactly for plain f16x3 planes and LDS-DMA images."""
    import torch
    plain = {"f32": torch.float32, "bf16x6": torch.bfloat16, "f16x3": torch.float16}
    for kind in D.DENSE_KINDS:
        w = torch.empty(0, dtype=plain[kind]) if kind in plain else D.F16x3Packed(kind, None, 128, 9, 32)
        assert D.dense_kind(w) == kind
        assert D.gap_fusable(w) == (kind in ("f16x3", "dma"))
