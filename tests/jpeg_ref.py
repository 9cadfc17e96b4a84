"""The rule of the project's baseline JPEG encoder (include/prisma_bands.h pb_jpeg_encode), restated in exact integers: written from ITU-T T.81
and the JFIF note, sharing no code with prisma_amd/csrc/jpeg.hip.  A helper module like tests/yuv_out_ref.py, not a conftest.

  input     one frame's planes as pb_rgb_to_yuv of {chroma, 8, full_range = 1, PB_YUV_BT601} lays them out: H W bytes of Y, then for 444 H W each
            of Cb and Cr, for 420 ceil(H / 2) ceil(W / 2) each; 400 has Y alone
  padding   every plane to whole MCUs (8 x 8 samples; 16 x 16 of Y and 8 x 8 of Cb / Cr at 420) by repeating its last column and row; minus 128
  DCT       F = C s C^T with the integer matrix C[u][x] = round(2^S c(u) / 2 cos((2x + 1) u pi / 16)), c(0) = 1 / sqrt 2, c(u) = 1; S = 13; no
            rounding between the passes, so F carries 2 S fractional bits
  quantise  round half away from zero of F / (2^(2S) Q): sign(F) ((|F| + D / 2) div D), D = Q 2^(2S), one integer division
  tables    Annex K.1 / K.2 scaled by quality 1 .. 100 as IJG does: s = 5000 div q below 50, else 200 - 2 q; (base s + 50) div 100 clamped to
            1 .. 255; Huffman tables Annex K.3 - K.6
  order     zigzag, then the entropy coder of F.1.2: DC difference to the previous block of the component inside the restart interval (0 at its
            start), AC as (run, size) with ZRL and EOB
  stream    SOI, APP0 (JFIF 1.01, density 1 : 1, no thumbnail), one DQT per table, SOF0 (components 1 2 3; sampling 1x1, or 2x2 1x1 1x1), one DHT
            per table (DC then AC, luminance then chrominance; 400 carries the luminance pair only), DRI = the MCUs of one MCU row, SOS, the
            intervals with RST(m mod 8) between interval m and m + 1, each padded to a byte with 1-bits and 0xFF stuffed with 0x00, EOI

`fault=` plants one mistake an implementation can make (FAULTS): tests show that each changes the bytes."""
import math

import numpy as np

S = 13

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

# Annex K.1 (luminance) and K.2 (chrominance), natural order
K1 = (16, 11, 10, 16, 24, 40, 51, 61,
      12, 12, 14, 19, 26, 58, 60, 55,
      14, 13, 16, 24, 40, 57, 69, 56,
      14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77,
      24, 35, 55, 64, 81, 104, 113, 92,
      49, 64, 78, 87, 103, 121, 120, 101,
      72, 92, 95, 98, 112, 100, 103, 99)
K2 = (17, 18, 24, 47, 99, 99, 99, 99,
      18, 21, 26, 66, 99, 99, 99, 99,
      24, 26, 56, 99, 99, 99, 99, 99,
      47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# Annex K.3 - K.6: (BITS: codes of each length 1 .. 16, HUFFVAL)
DC_LUM = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHR = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUM = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), tuple(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHR = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6"
    "c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
HUFF = {(0, 0): DC_LUM, (1, 0): AC_LUM, (0, 1): DC_CHR, (1, 1): AC_CHR}      # (class, id) as a DHT names them

CHROMAS = (444, 420, 400)
FAULTS = ("trunc_quant", "no_stuffing", "zero_pad", "dc_across_restart", "rst_unwrapped", "zero_edge", "chroma_tables_swapped")


def quant_tables(quality):
    """(luminance, chrominance) tables of a quality 1 .. 100, natural order"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality %r: 1 .. 100" % (quality,))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(max((b * s + 50) // 100, 1), 255) for b in base) for base in (K1, K2))


def cos_matrix(bits=S):
    """int64 [8, 8]: C[u][x] = round(2^bits c(u) / 2 cos((2x + 1) u pi / 16))"""
    return np.array([[round(2 ** bits * (math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16)) for x in range(8)]
                     for u in range(8)], np.int64)


def components(chroma):
    """[(id, h, v, table)] of a layout: sampling factors and the quantisation / Huffman table id"""
    if chroma == 400:
        return [(1, 1, 1, 0)]
    if chroma == 444:
        return [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    if chroma == 420:
        return [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    raise ValueError("chroma %r: one of %r" % (chroma, CHROMAS))


def mcu_grid(chroma, H, W):
    """(MCU rows, MCUs per row)"""
    m = 16 if chroma == 420 else 8
    return (H + m - 1) // m, (W + m - 1) // m


def split_planes(planes, H, W, chroma):
    """the frame's planes as uint8 2-D arrays"""
    a = np.frombuffer(bytes(planes), np.uint8) if not isinstance(planes, np.ndarray) else np.ascontiguousarray(planes, np.uint8).reshape(-1)
    ch, cw = ((H + 1) // 2, (W + 1) // 2) if chroma == 420 else (H, W)
    need = H * W + (0 if chroma == 400 else 2 * ch * cw)
    if a.size != need:
        raise ValueError("%d bytes for a %d x %d frame of %d: %d" % (a.size, H, W, chroma, need))
    out = [a[:H * W].reshape(H, W)]
    if chroma != 400:
        out += [a[H * W:H * W + ch * cw].reshape(ch, cw), a[H * W + ch * cw:].reshape(ch, cw)]
    return out


def pad_plane(p, bh, bw, fault=None):
    """int64 [8 bh, 8 bw]: the plane padded to whole blocks with its last column and row, minus 128"""
    h, w = p.shape
    if fault == "zero_edge":
        out = np.zeros((8 * bh, 8 * bw), np.int64)
        out[:h, :w] = p
    else:
        out = p[np.minimum(np.arange(8 * bh), h - 1)[:, None], np.minimum(np.arange(8 * bw), w - 1)[None, :]].astype(np.int64)
    return out - 128


def dct_blocks(padded, bits=S):
    """int64 [bh, bw, 8, 8] (v, u): F = C s C^T of every block, 2 bits fractional bits"""
    bh, bw = padded.shape[0] // 8, padded.shape[1] // 8
    blk = padded.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    C = cos_matrix(bits)
    return np.einsum("vy,abyx,ux->abvu", C, blk, C)


def quantise(F, table, bits=S, fault=None):
    """int64 [bh, bw, 8, 8]: round half away from zero of F / (2^(2 bits) Q)"""
    D = np.array(table, np.int64).reshape(8, 8) << (2 * bits)
    mag = np.abs(F) // D if fault == "trunc_quant" else (np.abs(F) + D // 2) // D
    return np.sign(F) * mag


def coefficients(planes, H, W, chroma, quality, fault=None):
    """per component int64 [bh, bw, 64]: the quantised coefficients in zigzag order"""
    rows, cols = mcu_grid(chroma, H, W)
    tabs = quant_tables(quality)
    out = []
    for p, (_, h, v, t) in zip(split_planes(planes, H, W, chroma), components(chroma)):
        q = quantise(dct_blocks(pad_plane(p, rows * v, cols * h, fault)), tabs[t], fault=fault)
        out.append(q.reshape(rows * v, cols * h, 64)[:, :, list(ZIGZAG)])
    return out


def huff_codes(bits, vals):
    """{symbol: (code, length)} of a table (Annex C)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _size_bits(v):
    """(category, the category's extra bits) of a value"""
    n = abs(v).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def flush(self, pad_ones=True):
        pad = -self.n % 8
        self.acc = (self.acc << pad) | ((1 << pad) - 1 if pad_ones else 0)
        self.n += pad
        return self.acc.to_bytes(self.n // 8, "big")


def encode_block(bw, zz, pred, dc, ac):
    """one block's codes (F.1.2) into the bit writer; returns its DC value"""
    n, extra = _size_bits(int(zz[0]) - pred)
    bw.put(*dc[n])
    bw.put(extra, n)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        n, extra = _size_bits(v)
        bw.put(*ac[(run << 4) | n])
        bw.put(extra, n)
        run = 0
    if run:
        bw.put(*ac[0x00])
    return int(zz[0])


def header(H, W, chroma, quality):
    """every byte of a frame before its entropy-coded data"""
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("%d x %d: a JPEG side is 1 .. 65535" % (H, W))
    comps = components(chroma)
    seg = lambda m, body: bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + body      # noqa: E731
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    tabs = quant_tables(quality)
    ntab = 1 if chroma == 400 else 2
    for t in range(ntab):
        out += seg(0xDB, bytes([t]) + bytes(tabs[t][z] for z in ZIGZAG))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([len(comps)])
               + b"".join(bytes([i, (h << 4) | v, t]) for i, h, v, t in comps))
    for t in range(ntab):
        for cls in (0, 1):
            bits, vals = HUFF[(cls, t)]
            out += seg(0xC4, bytes([(cls << 4) | t]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, mcu_grid(chroma, H, W)[1].to_bytes(2, "big"))
    out += seg(0xDA, bytes([len(comps)]) + b"".join(bytes([i, (t << 4) | t]) for i, _, _, t in comps) + b"\x00\x3f\x00")
    return out


def encode(planes, H, W, chroma, quality, fault=None):
    """the bytes of one frame: a complete .jpg"""
    if fault is not None and fault not in FAULTS:
        raise ValueError("fault %r: one of %r" % (fault, FAULTS))
    comps = components(chroma)
    coef = coefficients(planes, H, W, chroma, quality, fault)
    rows, cols = mcu_grid(chroma, H, W)
    tid = (lambda t: 1 - t) if fault == "chroma_tables_swapped" else (lambda t: t)
    dc = [huff_codes(*HUFF[(0, tid(t))]) for _, _, _, t in comps]
    ac = [huff_codes(*HUFF[(1, tid(t))]) for _, _, _, t in comps]
    out = [header(H, W, chroma, quality)]
    pred = [0] * len(comps)
    for r in range(rows):
        if r:
            out.append(bytes([0xFF, (0xD0 + ((r - 1) if fault == "rst_unwrapped" else (r - 1) % 8)) & 0xFF]))
        if fault != "dc_across_restart":
            pred = [0] * len(comps)
        bw = _Bits()
        for m in range(cols):
            for c, (_, h, v, _) in enumerate(comps):
                for dy in range(v):
                    for dx in range(h):
                        pred[c] = encode_block(bw, coef[c][r * v + dy, m * h + dx], pred[c], dc[c], ac[c])
        data = bw.flush(pad_ones=fault != "zero_pad")
        out.append(data if fault == "no_stuffing" else data.replace(b"\xff", b"\xff\x00"))
    out.append(b"\xff\xd9")
    return b"".join(out)


def encode_frames(planes, H, W, chroma, quality):
    """[n, frame bytes] uint8 (or one frame) -> the list of each frame's bytes: the encoder callable a VideoWriter takes"""
    a = np.ascontiguousarray(planes, np.uint8)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    return [encode(f, H, W, chroma, quality) for f in a]
