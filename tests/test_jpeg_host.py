"""CPU suite: the host half of the split JPEG decoder (csrc/jpeg_host.cpp: no GPU needed) + the numpy restatement of the
device half (oracle/jpeg_oracle.py) == the INSTALLED Pillow's decode, byte for byte -- which pins both: the entropy decoder's
coefficients cannot be read out of Pillow, so they are checked through the pixels they produce.  Images: the seeded synthetic
camera frames of the file-pool tests, written by Pillow itself at several qualities / subsamplings / sizes that are not
multiples of the MCU, with restart intervals, grayscale; unsupported streams (progressive) must be REFUSED, not mis-decoded.

The layouts Pillow's encoder cannot write (4:4:0, Cb and Cr with different factors, chroma at full resolution), restart
intervals in MCUs, streams without JFIF and with fill bytes come from tests/jpeg_encode.py, a numpy baseline writer that is
itself pinned by Pillow here.  Every stream the decoder ACCEPTS must equal Pillow; what it cannot decode as Pillow does (a
scan that ends early, a missing EOI, narrow subsampled frames, 16-bit tables) must be refused, so that the loader hands the
file to Pillow."""
import ctypes
import functools
import io
import warnings

import numpy as np
import pytest

import jpeg_encode as JE
import jpeg_oracle as JO
from gen_golden_bevfusion_loading import synth_image


def _encode(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _pil(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def host_decode(data):
    from al3d import lib
    L = lib.load()
    info = (ctypes.c_int * 32)()
    quant = (ctypes.c_uint16 * 192)()
    buf = (ctypes.c_ubyte * len(data)).from_buffer_copy(data)
    lib.call("al3d_jpeg_header", buf, len(data), info, quant)
    coefs = np.empty((info[20], 64), np.int16)
    lib.call("al3d_jpeg_entropy_decode", buf, len(data), coefs.ctypes.data_as(ctypes.c_void_p), info[20])
    return np.array(info[:]), np.array(quant[:], dtype=np.uint16).reshape(3, 64), coefs


CASES = [
    dict(hw=(225, 400), kw=dict(quality=75)),                                   # 4:2:0, height not a multiple of 16
    dict(hw=(231, 417), kw=dict(quality=90)),                                   # odd sizes
    dict(hw=(64, 48), kw=dict(quality=30)),
    dict(hw=(97, 131), kw=dict(quality=95, subsampling=0)),                     # 4:4:4
    dict(hw=(97, 131), kw=dict(quality=85, subsampling=1)),                     # 4:2:2
    dict(hw=(120, 160), kw=dict(quality=75, optimize=True)),                    # optimised Huffman tables
    dict(hw=(900, 1600), kw=dict(quality=75)),                                  # a camera frame of the pool
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_entropy_decode_plus_oracle_equals_pillow(case):
    c = CASES[case]
    img = synth_image(10 + case, *c["hw"])
    data = _encode(img, **c["kw"])
    want = _pil(data)
    info, quant, coefs = host_decode(data)
    assert (info[0], info[1]) == (c["hw"][1], c["hw"][0])
    got = JO.decode(info, quant, coefs)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_grayscale_and_restart_intervals():
    from PIL import Image
    g = synth_image(3, 75, 101)[..., 0]
    buf = io.BytesIO()
    Image.fromarray(g).save(buf, format="JPEG", quality=80)
    info, quant, coefs = host_decode(buf.getvalue())
    assert info[2] == 1 and np.array_equal(JO.decode(info, quant, coefs), _pil(buf.getvalue()))
    # restart intervals written by Pillow's encoder: every 1, 3, 8, 64 MCUs and one per MCU row
    img = synth_image(5, 120, 200)
    for kw, ri in ((dict(restart_marker_blocks=1), 1), (dict(restart_marker_blocks=3), 3), (dict(restart_marker_blocks=8), 8),
                   (dict(restart_marker_blocks=64), 64), (dict(restart_marker_rows=1), 13)):
        data = _encode(img, quality=75, **kw)
        info, quant, coefs = host_decode(data)
        assert info[21] == ri, kw
        assert np.array_equal(JO.decode(info, quant, coefs), _pil(data)), kw


def test_unsupported_streams_are_refused():
    from al3d import lib
    img = synth_image(7, 64, 64)
    data = _encode(img, quality=75, progressive=True)
    info = (ctypes.c_int * 32)()
    quant = (ctypes.c_uint16 * 192)()
    buf = (ctypes.c_ubyte * len(data)).from_buffer_copy(data)
    with pytest.raises(lib.Al3dError, match="SOF2|baseline"):
        lib.call("al3d_jpeg_header", buf, len(data), info, quant)
    with pytest.raises(lib.Al3dError):
        lib.call("al3d_jpeg_header", (ctypes.c_ubyte * 4)(1, 2, 3, 4), 4, info, quant)


def test_mutated_files_are_refused_or_decoded_never_fatal():
    """Untrusted input: bit flips, truncations and overwritten header bytes of valid files must end in an error code or a
    decode, never in a crash or an out-of-bounds access (the same mutations run under AddressSanitizer + UBSan in
    tools/fuzz/run_jpeg_fuzz.sh: 28,000 inputs, no finding)."""
    import ctypes
    import io
    from PIL import Image
    from al3d import lib
    L = lib.load()
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:61, 0:83]
    img = np.stack([(xx * 3) % 256, (yy * 5) % 256, ((xx + yy) * 7) % 256], -1).astype(np.uint8)
    refused = decoded = 0
    for sub in (0, 1, 2):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=80, subsampling=sub)
        base = np.frombuffer(buf.getvalue(), dtype=np.uint8)
        for it in range(150):
            d = base.copy()
            mode = it % 3
            if mode == 0:
                for _ in range(int(rng.integers(1, 8))):
                    d[rng.integers(0, d.size)] ^= np.uint8(1 << rng.integers(0, 8))
            elif mode == 1:
                d = d[:int(rng.integers(1, d.size))].copy()
            else:
                for _ in range(int(rng.integers(1, 6))):
                    d[rng.integers(0, min(d.size, 700))] = rng.integers(0, 256)
            info = (ctypes.c_int * 32)()
            quant = (ctypes.c_ushort * 192)()
            rc = L.al3d_jpeg_header(d.ctypes.data_as(ctypes.c_void_p), d.size, info, quant)
            if rc == 0 and 0 < info[20] < (1 << 20):
                coefs = np.empty((info[20], 64), dtype=np.int16)
                rc = L.al3d_jpeg_entropy_decode(d.ctypes.data_as(ctypes.c_void_p), d.size, coefs.ctypes.data_as(ctypes.c_void_p),
                                                info[20])
            refused += rc != 0
            decoded += rc == 0
    assert refused > 50 and decoded > 50          # both outcomes occur; reaching this line is the test


# ---- streams from the numpy writer (tests/jpeg_encode.py)

LAYOUTS = {                                                  # sampling factors (h, v) of Y, Cb, Cr
    "444": ((1, 1), (1, 1), (1, 1)),
    "422": ((2, 1), (1, 1), (1, 1)),
    "420": ((2, 2), (1, 1), (1, 1)),
    "440": ((1, 2), (1, 1), (1, 1)),                         # the h1v2 branch of the upsampler
    "cb2x1_cr1x2": ((2, 2), (2, 1), (1, 2)),                 # Cb h1v2, Cr h2v1 under a 16 x 16 MCU
    "cb2x2_cr1x1": ((2, 2), (2, 2), (1, 1)),                 # Cb at full resolution
    "cb1x1_cr2x1": ((2, 1), (1, 1), (2, 1)),
}
# restart intervals of 3 MCUs and of 1: at 61 x 83 the first wraps past RST7 with the 8-row MCUs only, the second always
VARIANTS = {"plain": dict(), "restart3": dict(restart=3), "restart1": dict(restart=1), "nojfif_fill": dict(jfif=False, fill=3)}
RAGGED = (61, 83)                                            # H, W: ragged against the 8x8, 16x8, 8x16 and 16x16 MCUs
# the smallest frames that reach every branch of the upsampler: H = 1, 2, 3, 4 (vertical ratio 2: the farther row clamps at both
# ends, at H = 1 and 2 both clamps coincide), W = 5, 6 (3 real chroma columns, the narrowest frame with fancy h2v1 / h2v2)
# H = 4 is the smallest frame in which the replica below the last real chroma row shows (at H = 3 that output row is cropped)
SMALL = [(h, w) for h in (1, 2, 3, 4) for w in (5, 6)]
_NATURAL = np.add.outer(np.arange(8), np.arange(8)).reshape(64)
QUANTS = [(8, 12), (4 + _NATURAL, 7 + 2 * _NATURAL)]         # flat tables; tables that grow with the frequency


def device_sizes(layout):
    return [RAGGED] + SMALL + ([(h, 1) for h in (1, 2, 3, 4)] if layout == "440" else [])


def picture(seed, H, W, steep=False):
    """Gradients plus noise, [H, W, 3] uint8.  steep: slopes at which the chroma of neighbouring rows and columns differs by
    tens of levels after quantisation, so that a frame of a few pixels still tells the upsampler's rounding and edge rules."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    if steep:
        img = np.stack([(xx * 37 + yy * 61) % 256, (yy * 53 + xx * 11 + 40) % 256, (xx * 87 + yy * 203) % 256], -1)
    else:
        img = np.stack([(xx * 3) % 256, (yy * 2 + 40) % 256, (xx + yy) % 256], -1)
    return (img + rng.integers(-12, 13, img.shape)).clip(0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def stream(layout, hw, k=0, variant="plain"):
    """(bytes, Pillow's decode) of picture k in this layout; computed once, shared by the CPU and the GPU tests."""
    data = JE.encode(picture(20 + k, *hw, steep=hw != RAGGED), LAYOUTS[layout], quant=QUANTS[k], **VARIANTS[variant])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # Pillow must open the writer's streams without a warning
        want = _pil(data)
    want.setflags(write=False)
    return data, want


def try_decode(data):
    """The oracle's pixels of what the host half accepts, or None when it refuses the stream."""
    from al3d import lib
    try:
        return JO.decode(*host_decode(data))
    except lib.Al3dError:
        return None


def _dht_payloads(data):
    out, i = [], 2
    while data[i + 1] != 0xda:
        n = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xc4:
            out.append(bytes(data[i + 4:i + 2 + n]))
        i += 2 + n
    return out


def test_writer_huffman_tables_are_annex_k():
    """The writer's tables are the ones Pillow (libjpeg) writes when it does not optimise: T.81 Annex K."""
    assert _dht_payloads(_encode(synth_image(1, 16, 16), quality=75)) == JE.ANNEX_K
    assert _dht_payloads(stream("420", RAGGED)[0]) == JE.ANNEX_K


def test_writer_is_pinned_by_pillow():
    """Every stream of the writer that these tests and tests/test_jpeg_gpu.py use opens in Pillow without a warning (stream()
    turns warnings into errors) and decodes close to its source picture.  Measured mean absolute error in grey levels:
      * 61 x 83, gentle gradients: 4.04 (4:4:4) to 5.38 (4:2:0) with the flat tables of 8 and 12, 5.12 (4:4:4) to 5.57 (4:2:0)
        with the tables that grow with the frequency;
      * the frames of at most 4 x 6 pixels, steep gradients: 0.33 (4:4:0, 1 x 1) to 8.00 without subsampling (4:4:4), up to
        33.96 (4:2:0, 4 x 6) with it -- there one chroma sample stands for pixels that differ by tens of levels.
    Each bound is twice the largest value measured in its group."""
    worst = {False: 0.0, True: 0.0}
    for layout in LAYOUTS:
        for hw in device_sizes(layout):
            for k in (0, 1):
                for variant in (VARIANTS if hw == RAGGED and k == 0 else ("plain",)):
                    data, got = stream(layout, hw, k, variant)
                    assert got.shape == hw + (3,)
                    steep = hw != RAGGED
                    mae = float(np.abs(got.astype(np.int64) - picture(20 + k, *hw, steep=steep)).mean())
                    print(f"{layout} {hw} picture {k} {variant}: {len(data)} bytes, mean abs error {mae:.2f}")
                    worst[steep] = max(worst[steep], mae)
    assert worst[False] <= 2 * 5.57 and worst[True] <= 2 * 33.96, worst


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts_pillow_cannot_write_equal_pillow(layout, variant):
    data, want = stream(layout, RAGGED, 0, variant)
    info, quant, coefs = host_decode(data)
    assert info[21] == VARIANTS[variant].get("restart", 0)
    if info[21]:
        markers = (info[9] * info[10] - 1) // info[21]
        assert sum(data.count(bytes([0xff, 0xd0 + k])) for k in range(8)) >= markers
        assert markers > 8 or variant == "restart3"          # RSTn wraps past RST7
    assert [(info[3 + c], info[6 + c]) for c in range(3)] == list(LAYOUTS[layout])
    assert np.array_equal(JO.decode(info, quant, coefs), want)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_small_frames_of_every_layout_equal_pillow(layout):
    """The frames tests/test_jpeg_gpu.py runs on the device, through the oracle: accepted, and equal to Pillow."""
    for hw in device_sizes(layout):
        for k in (0, 1):
            data, want = stream(layout, hw, k)
            assert np.array_equal(JO.decode(*host_decode(data)), want), (hw, k)


SWEEP = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 15, 16, 17, 31, 32, 33)


@pytest.mark.parametrize("sub", (0, 1, 2))
def test_size_sweep_is_refused_or_equal(sub):
    """Pillow-written files of every small size: each is refused (libjpeg replicates where a horizontally subsampled
    component has at most 2 real columns; the upsampler here is the fancy one only) or equal, and from W = 5 on accepted."""
    img = synth_image(31, 33, 33)
    refused = []
    for H in SWEEP:
        for W in SWEEP:
            data = _encode(img[:H, :W], quality=85, subsampling=sub)
            got = try_decode(data)
            if got is None:
                refused.append((H, W))
            else:
                assert np.array_equal(got, _pil(data)), (H, W)
    assert refused == ([] if sub == 0 else [(H, W) for H in SWEEP for W in (1, 2, 3, 4)])


def _scan_start(data):
    i = 2
    while data[i + 1] != 0xda:
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    return i + 2 + ((data[i + 2] << 8) | data[i + 3])


@pytest.mark.parametrize("variant", ("plain", "restart3"))
def test_scans_that_end_early_are_refused(variant):
    """Pillow raises 'image file is truncated' on a file cut anywhere, and leaves the MCUs after an early EOI zero: neither
    may come back as a decode.  Stray and fill bytes before the EOI are passed over, as libjpeg passes them."""
    from al3d import lib
    data, want = stream("420", RAGGED, 0, variant)
    start = _scan_start(data)
    assert data[-2:] == b"\xff\xd9" and len(data) - start > 1500
    for n in range(1, len(data)):                            # every proper prefix: header, scan, half an EOI
        assert try_decode(data[:n]) is None, n
    for n in range(start, len(data) - 2):                    # the scan cut anywhere, then EOI
        assert try_decode(data[:n] + b"\xff\xd9") is None, n
    with pytest.raises(lib.Al3dError, match="premature end of scan|restart marker"):
        host_decode(data[:start + 2 * (len(data) - start) // 3] + b"\xff\xd9")
    with pytest.raises(lib.Al3dError, match="no EOI"):
        host_decode(data[:-2])
    for stray in (b"\xff\xff\xff", b"\x00\x12\x34", b"\xff\x00\x80\xff"):
        assert np.array_equal(try_decode(data[:-2] + stray + b"\xff\xd9"), want), stray


def test_pillow_files_that_end_early_are_refused():
    from PIL import Image
    data = _encode(synth_image(9, 61, 83), quality=80)
    assert np.array_equal(try_decode(data), _pil(data))
    start = _scan_start(data)
    for n in range(start, len(data)):
        assert try_decode(data[:n]) is None, n
    cut = data[:start + 2 * (len(data) - start) // 3]
    with pytest.raises(OSError, match="truncated"):
        Image.open(io.BytesIO(cut)).convert("RGB")
    assert try_decode(cut + b"\xff\xd9") is None
    assert _pil(cut + b"\xff\xd9").shape == (61, 83, 3)      # Pillow decodes the early EOI: the loader returns its pixels


def test_411_and_16_bit_tables_are_refused_at_the_header():
    from al3d import lib
    info = (ctypes.c_int * 32)()
    quant = (ctypes.c_uint16 * 192)()
    img = picture(3, 24, 40)
    for data, why in ((JE.encode(img, ((4, 1), (1, 1), (1, 1))), "sampling factor 4 x 1"),
                      (JE.encode(img, LAYOUTS["420"], pq16=True), "16-bit quantisation table"),
                      (JE.encode(img, LAYOUTS["420"], quant=(300, 700), pq16=True), "16-bit quantisation table")):
        _pil(data)                                           # a stream Pillow decodes
        buf = (ctypes.c_ubyte * len(data)).from_buffer_copy(data)
        with pytest.raises(lib.Al3dError, match=why):
            lib.call("al3d_jpeg_header", buf, len(data), info, quant)
    ok = JE.encode(img, LAYOUTS["420"], ids=(0, 1, 2))       # other component ids are no reason to refuse
    assert np.array_equal(try_decode(ok), _pil(ok))
