"""CPU suite: detector_ops.sparse_structure over the 21 layers of FPNSpMiddleResNetFHD, under each arithmetic and the
dispatch settings the GPU tests set.  The expected lists are the al3d_sp_conv_* launches the encoder made before its
dispatch moved behind sparse_structure."""
import pytest

from al3d import detector_ops as D

# (cin, cout, K, subm) in plan order: level 0 (5 -> 16, four 16 -> 16), 16 -> 32 strided, level 1, 32 -> 64, level 2,
# 64 -> 128, level 3, the (3, 1, 1) strided 128 -> 128
LAYERS = ([(5, 16, 27, True)] + [(16, 16, 27, True)] * 4 + [(16, 32, 27, False)] + [(32, 32, 27, True)] * 4 +
          [(32, 64, 27, False)] + [(64, 64, 27, True)] * 4 + [(64, 128, 27, False)] + [(128, 128, 27, True)] * 4 +
          [(128, 128, 3, False)])
SETTINGS = ("MATH", "SPCONV", "L0", "R16_COUTS", "GLDS_PAIRS", "RNG_PAIRS", "BLK_PAIRS", "BLK_ORDER_ONLY")
P3 = {(32, 32), (64, 64), (128, 128)}
T, G, R, B = "wave2_f16x3_tiles", "glds_f16x3", "rng_f16x3", "blk_f16x3"
L0 = ["r16_f16x3"] * 5 + [T]


def _levels(l1, l2, l3, last=T):
    """f16x3 list with the default level 0: l1 / l2 / l3 = the four submanifold layers of levels 1-3."""
    return L0 + [l1] * 4 + [T] + [l2] * 4 + [T] + [l3] * 4 + [last]


CASES = [
    (dict(), _levels(R, G, T)),
    (dict(MATH="bf16x6"), ["wave2"] * 21),
    (dict(MATH="f32"), [False] + [True] * 20),
    (dict(SPCONV="glds"), [G] * 21),
    (dict(SPCONV="rng"), [T] * 6 + [R] * 4 + [T] + [R] * 4 + [T] * 6),
    (dict(SPCONV="wave2"), [T] * 21),
    (dict(MATH="bf16x6", SPCONV="wave"), ["wave"] * 21),
    (dict(MATH="bf16x6", SPCONV="tile"), ["bf16x6"] * 21),
    (dict(L0="off"), [T] * 6 + _levels(R, G, T)[6:]),
    (dict(R16_COUTS={16, 32}), ["r16_f16x3"] * 6 + _levels(R, G, T)[6:]),
    (dict(R16_COUTS=set()), [T] * 6 + _levels(R, G, T)[6:]),
    (dict(BLK_PAIRS={(32, 32)}), _levels(B, G, T)),
    (dict(BLK_PAIRS={(64, 64)}), _levels(R, B, T)),
    (dict(BLK_PAIRS={(128, 128)}), _levels(R, G, B)),
    (dict(BLK_PAIRS=P3), _levels(B, B, B)),
    (dict(BLK_PAIRS=P3, BLK_ORDER_ONLY=True), _levels(R, G, T)),
    (dict(GLDS_PAIRS=P3), _levels(R, G, G, G)),
    (dict(RNG_PAIRS=set()), _levels(G, G, T)),
    (dict(RNG_PAIRS={(32, 32), (64, 64)}), _levels(R, R, T)),
]


@pytest.fixture
def settings():
    saved = {k: getattr(D, k) for k in SETTINGS}
    defaults = dict(MATH="f16x3", SPCONV="auto", L0="raster", R16_COUTS={16}, GLDS_PAIRS={(32, 32), (64, 64)},
                    RNG_PAIRS={(32, 32)}, BLK_PAIRS=set(), BLK_ORDER_ONLY=False)
    try:
        for k, v in defaults.items():
            setattr(D, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(D, k, v)


@pytest.mark.parametrize("overrides,want", CASES, ids=[",".join(f"{k}={v}" for k, v in c.items()) or "default"
                                                        for c, _ in CASES])
def test_encoder_structures(settings, overrides, want):
    for k, v in overrides.items():
        setattr(D, k, v)
    got = [D.sparse_structure(cin, cout, K, subm, True) for cin, cout, K, subm in LAYERS]
    assert [name for name, _, _ in got] == want
    # the narrow first layer runs zero-padded to 16 channels on the matrix cores, at 5 on the f32 VALU kernel
    assert [cin for _, cin, _ in got] == [5 if D.MATH == "f32" else 16] + [c for c, _, _, _ in LAYERS[1:]]
    # column order for the levels whose layers are block-staged, also when only the order is kept
    blk = D.BLK_PAIRS & D.BLK_BUILT if D.MATH == "f16x3" and D.SPCONV == "auto" else set()
    assert [cols for _, _, cols in got] == [subm and K == 27 and (cin, cout) in blk for cin, cout, K, subm in LAYERS]


def test_rows_in_caller_order_never_take_the_item_stream_kernel(settings):
    """sparse_conv_layer's default (raster_ok=False): level 0 on the register-gather wave kernel's tiled table."""
    got = [D.sparse_structure(cin, cout, K, subm, False)[0] for cin, cout, K, subm in LAYERS]
    assert got == [T] * 6 + _levels(R, G, T)[6:]


def test_every_structure_is_described_once():
    """Pair rows (io) and side data exist for the tiled f16x3 kernels only."""
    assert len({fn for fn, _, _, _ in D.SPARSE.values()}) == len(D.SPARSE) == 11
    for name, (fn, fmt, tiled, side) in D.SPARSE.items():
        assert fn.startswith("al3d_sp_conv_")
        assert tiled == (fmt in ("f16x3", "glds", "r16") and name != "wave2_f16x3")
        assert side is None or tiled
