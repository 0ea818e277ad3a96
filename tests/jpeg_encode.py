"""TEST INFRASTRUCTURE ONLY -- never imported by the product path.

A small baseline (SOF0) JPEG writer in numpy, for the streams Pillow's encoder cannot write: arbitrary sampling factors per
component (4:4:0, Cb and Cr with different factors, chroma at full resolution), restart intervals in MCUs, no JFIF segment,
0xFF fill bytes before markers, 16-bit quantisation tables, other component ids.  One interleaved scan, the Huffman tables of
ITU-T T.81 Annex K (tests/test_jpeg_host.py checks them against the DHT segments Pillow writes).  It is pinned by Pillow only:
Pillow opens what it writes without a warning and decodes it close to the source image.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])

# Annex K.3: the payloads of the four DHT tables (Tc/Th byte, 16 counts, the values), luma DC / AC then chroma DC / AC
ANNEX_K = [bytes.fromhex(h) for h in (
    "00" "00010501010101010100000000000000" "000102030405060708090a0b",
    "10" "0002010303020403050504040000017d"
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa",
    "01" "00030101010101010101010000000000" "000102030405060708090a0b",
    "11" "00020102040403040705040400010277"
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536373839"
    "3a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7"
    "a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")]


def _codes(table):
    """DHT payload -> {symbol: (code, length)} (T.81 Annex C)."""
    out, code, k = {}, 0, 17
    for length in range(1, 17):
        for _ in range(table[length]):
            out[table[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


_DC = [_codes(ANNEX_K[0]), _codes(ANNEX_K[2])]
_AC = [_codes(ANNEX_K[1]), _codes(ANNEX_K[3])]
_k = np.arange(8)
_C = np.sqrt(0.25) * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16)     # orthonormal DCT-II = the JPEG FDCT
_C[0] = np.sqrt(0.125)


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)                           # byte stuffing
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)    # pad the last byte with ones


def _value(bits, v, table, sym_hi):
    s = int(abs(v)).bit_length()
    bits.put(*table[sym_hi | s])
    if s:
        bits.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)


def _block(bits, zz, pred, dc, ac):
    _value(bits, int(zz[0]) - pred, dc, 0)
    run = 0
    last = int(np.max(np.nonzero(zz)[0], initial=0))
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])                              # ZRL
            run -= 16
        _value(bits, int(zz[k]), ac, run << 4)
        run = 0
    if last < 63:
        bits.put(*ac[0x00])                                  # EOB
    return int(zz[0])


def _segment(marker, payload, fill):
    return b"\xff" * fill + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def encode(img, samp=((2, 2), (1, 1), (1, 1)), quant=(8, 12), pq16=False, restart=0, jfif=True, fill=0, ids=(1, 2, 3)):
    """img [H, W, 3] uint8 RGB -> the bytes of a baseline JPEG with one interleaved scan.

    samp     (h, v) sampling factors of Y, Cb, Cr (each 1 or 2 for what the product decodes; anything T.81 allows is written)
    quant    two quantisation tables, luma and chroma: a number (flat table) or 64 values in natural order
    pq16     write the tables with 16-bit entries (Pq = 1)
    restart  restart interval in MCUs (0: none); RSTn wraps past RST7
    jfif     write the JFIF APP0 segment
    fill     number of 0xFF fill bytes in front of every marker after SOI
    ids      the three component ids
    """
    img = np.asarray(img)
    H, W = img.shape[:2]
    mh, mv = max(s[0] for s in samp), max(s[1] for s in samp)
    mx, my = -(-W // (8 * mh)), -(-H // (8 * mv))
    rgb = np.pad(img.astype(np.float64), ((0, my * 8 * mv - H), (0, mx * 8 * mh - W), (0, 0)), mode="edge")
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    ycc = [0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128,
           0.5 * r - 0.418688 * g - 0.081312 * b + 128]
    qt = [np.broadcast_to(np.asarray(q, np.int64).reshape(-1), (64,)) for q in quant]
    blocks = []                                              # per component [block rows, blocks per row, 64] in zigzag order
    for c, (h, v) in enumerate(samp):
        fh, fv = mh // h, mv // v
        p = ycc[c].reshape(my * 8 * v, fv, mx * 8 * h, fh).mean((1, 3)) - 128
        p = p.reshape(my * v, 8, mx * h, 8).transpose(0, 2, 1, 3)
        co = np.rint((_C @ p @ _C.T).reshape(my * v, mx * h, 64) / qt[min(c, 1)]).astype(np.int64)
        blocks.append(co[..., ZIGZAG])
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += _segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0", fill)
    for t in (0, 1):
        zz = qt[t][ZIGZAG]
        body = b"".join(int(x).to_bytes(2, "big") for x in zz) if pq16 else bytes(int(x) for x in zz)
        out += _segment(0xDB, bytes([(16 if pq16 else 0) | t]) + body, fill)
    sof = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3])
    for c, (h, v) in enumerate(samp):
        sof += bytes([ids[c], (h << 4) | v, min(c, 1)])
    out += _segment(0xC0, sof, fill)
    for t in ANNEX_K:
        out += _segment(0xC4, t, fill)
    if restart:
        out += _segment(0xDD, int(restart).to_bytes(2, "big"), fill)
    out += _segment(0xDA, bytes([3, ids[0], 0x00, ids[1], 0x11, ids[2], 0x11, 0, 63, 0]), fill)
    bits, pred, n = _Bits(), [0, 0, 0], 0
    for y in range(my):
        for x in range(mx):
            if restart and n and n % restart == 0:
                bits.flush()
                out += bits.out + b"\xff" * fill + bytes([0xFF, 0xD0 + (n // restart - 1) % 8])
                bits, pred = _Bits(), [0, 0, 0]
            for c, (h, v) in enumerate(samp):
                for by in range(v):
                    for bx in range(h):
                        pred[c] = _block(bits, blocks[c][y * v + by, x * h + bx], pred[c], _DC[min(c, 1)], _AC[min(c, 1)])
            n += 1
    bits.flush()
    return bytes(out + bits.out + b"\xff" * fill + b"\xff\xd9")
