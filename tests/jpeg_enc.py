"""A minimal baseline JPEG encoder with caller-chosen Huffman tables (test
infrastructure): Pillow / libjpeg-turbo always writes either the Annex K
tables or optimised ones, whose codes longer than 11 bits all lie in the top
1/64 of the 16-bit code space -- so no Pillow file reaches the device entropy
decoder's searching path (jpeghuff.hip Dec::step, HuffDev::search).  This
writes files whose tables put long codes far below that (DEEP_DC / DEEP_AC),
so the tests can decode them on the GPU and compare with the host decoder and
with Pillow.  Pixels go through a float DCT and a flat quantiser; the result
only has to be a valid JPEG (every decoder reads the same file)."""
import numpy as np

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63])

# DC categories 0..11: three 2-bit codes, one 3-bit code, the other eight
# 12-bit codes starting at 1110 0000 0000 (11-bit prefix 1792 < 2016).
DEEP_DC = ([0, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])
# AC: EOB / 0x01 / 0x02 at 2 bits, six 5-bit codes, the other 153 symbols at
# 12 bits starting at 1111 0000 0000 (11-bit prefix 1920 < 2016).
_AC_SHORT = [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x21, 0x05, 0xF0]
_AC_ALL = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
DEEP_AC = ([0, 3, 0, 0, 6, 0, 0, 0, 0, 0, 0, 153, 0, 0, 0, 0], _AC_SHORT + [v for v in _AC_ALL if v not in _AC_SHORT])

# Further tables, so one scan can name four distinct DC and four distinct AC
# tables: the deep shapes with other symbols on the short codes, fixed-length
# codes (no code past the look-up), and T.81 Annex K's luminance code lengths
# (codes up to 16 bits, all in the top of the code space) over this module's
# own symbol order.
DEEP_DC2 = (DEEP_DC[0], list(range(11, -1, -1)))
_AC_SHORT2 = [0x00, 0x01, 0x11, 0x02, 0x03, 0x12, 0x21, 0x31, 0x41]
DEEP_AC2 = (DEEP_AC[0], _AC_SHORT2 + [v for v in _AC_ALL if v not in _AC_SHORT2])
FLAT_DC = ([0, 0, 0, 12, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
FLAT_AC = ([0, 0, 0, 0, 0, 0, 0, 162, 0, 0, 0, 0, 0, 0, 0, 0], _AC_ALL)
LONG_DC = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
LONG_AC = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [0x00] + sorted((v for v in _AC_ALL if v), key=lambda v: ((v >> 4) + 2 * (v & 15), v)))
DC_TABLES = [DEEP_DC, FLAT_DC, DEEP_DC2, LONG_DC]
AC_TABLES = [DEEP_AC, FLAT_AC, DEEP_AC2, LONG_AC]


def first_long_prefix(counts):
    """The 11-bit prefix of the first code longer than 11 bits (2048: none) --
    the device decoder searches a table when it is below 2016."""
    code = 0
    for n in range(1, 17):
        if n > 11 and counts[n - 1]:
            return (code << (16 - n)) >> 5
        code = (code + counts[n - 1]) << 1
    return 2048


def _codes(table):
    counts, vals = table
    out, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(counts[n - 1]):
            out[vals[k]] = (code, n)
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    """Bits, most significant first, into .out with 0xFF bytes stuffed."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.n += n
        if self.n >= 512:
            self._drain()

    def _drain(self):
        k = self.n & 7
        self.out += (self.acc >> k).to_bytes(self.n >> 3, "big").replace(b"\xff", b"\xff\x00")
        self.acc &= (1 << k) - 1
        self.n = k

    def flush(self):
        if self.n & 7:
            self.put((1 << (8 - (self.n & 7))) - 1, 8 - (self.n & 7))
        self._drain()


def _category(v):
    return int(abs(int(v))).bit_length()


def _dct_blocks(plane, q, grid=None):
    """(rows, cols, 64) quantised coefficients in zigzag order; grid: the
    (rows, cols) of blocks to pad the plane to (default: what covers it)."""
    h, w = plane.shape
    ph, pw = (-(-h // 8) * 8, -(-w // 8) * 8) if grid is None else (grid[0] * 8, grid[1] * 8)
    p = np.pad(plane.astype(np.float64), ((0, ph - h), (0, pw - w)), mode="edge") - 128.0
    k = np.arange(8)
    c = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k == 0, np.sqrt(1 / 8), 0.5)[:, None]
    b = p.reshape(ph // 8, 8, pw // 8, 8).transpose(0, 2, 1, 3)
    f = np.einsum("ij,rcjk,lk->rcil", c, b, c)
    z = np.rint(f / q).astype(np.int64).reshape(ph // 8, pw // 8, 64)[:, :, ZIGZAG]
    return np.clip(z, -1023, 1023)


def _subsample(plane, dh, dw, vx, hx):
    """Every vx-th row and hx-th column of a full-size plane, (dh, dw) samples."""
    h, w = plane.shape
    if (dh, dw, vx, hx) == (h, w, 1, 1):
        return plane  # as given (a copy's other memory layout can move a float DCT's rounding ties)
    ys = np.minimum(np.arange(dh) * vx, h - 1)
    xs = np.minimum(np.arange(dw) * hx, w - 1)
    return plane[ys][:, xs]


def encode(pixels, dc=DEEP_DC, ac=DEEP_AC, q=2, restart_mcus=0, coefs=None, adobe=None, sampling=None, tables=None):
    """pixels: (H, W) or (H, W, C) uint8 -> baseline JPEG bytes; the
    components are written as given (Y, Cb, Cr when three).  q: the flat
    quantiser (int) or a 64-entry table in natural order.  coefs: the
    quantised blocks to write instead of the pixels' -- per component a
    (rows, cols, 64) zig-zag array (DC within +-2047 of its neighbour, AC
    within +-1023) covering the component's padded block grid -- pixels then
    only gives the frame size.  adobe: write an Adobe APP14 marker with this
    colour transform (0: RGB / CMYK as stored, 1: YCbCr, 2: YCCK for four
    components).

    sampling: (h, v) per component (default all (1, 1)).  Component i holds
    ceil(W h / max_h) x ceil(H v / max_v) samples (point-sampled from the
    full-size plane) padded to the MCU grid, mcux h x mcuy v blocks, and the
    scan is interleaved: per MCU and component v rows of h blocks.  A
    one-component file is not interleaved (T.81 A.2.2): ceil(W / 8) x
    ceil(H / 8) blocks in raster order, its factors written in SOF only.
    restart_mcus counts MCUs of the scan's order.

    tables: (quantiser id, DC table id, AC table id) per component; q, dc
    and ac are then sequences indexed by those ids (up to four each), all of
    them written to the file.  Default: one of each, id 0."""
    a = pixels if pixels.ndim == 3 else pixels[:, :, None]
    h, w, nc = a.shape
    samp = [(1, 1)] * nc if sampling is None else [tuple(s) for s in sampling]
    assert len(samp) == nc and all(1 <= sh <= 4 and 1 <= sv <= 4 for sh, sv in samp)
    if tables is None:
        ids, qs, dcs, acs = [(0, 0, 0)] * nc, [q], [dc], [ac]
    else:
        ids, qs, dcs, acs = [tuple(t) for t in tables], list(q), list(dc), list(ac)
        assert len(ids) == nc and max(len(qs), len(dcs), len(acs)) <= 4
    qts = [np.full(64, x, np.int64) if np.isscalar(x) else np.asarray(x, np.int64) for x in qs]
    max_h, max_v = max(s[0] for s in samp), max(s[1] for s in samp)
    mcux, mcuy = -(-w // (8 * max_h)), -(-h // (8 * max_v))
    if nc == 1:  # non-interleaved: one block per MCU, the factors ignored
        grids, per_mcu, mcux, mcuy = [None], [(1, 1)], -(-w // 8), -(-h // 8)
    else:
        grids, per_mcu = [(mcuy * sv, mcux * sh) for sh, sv in samp], samp
    if coefs is not None:
        planes = coefs
    else:
        planes = []
        for i, (sh, sv) in enumerate(samp):
            if nc == 1:
                p = a[:, :, 0]
            else:
                p = _subsample(a[:, :, i], -(-h * sv // max_v), -(-w * sh // max_h), max_v // sv, max_h // sh)
            planes.append(_dct_blocks(p, qts[ids[i][0]].reshape(8, 8), grids[i]))
    rows, cols = mcuy, mcux
    dccs, accs = [_codes(t) for t in dcs], [_codes(t) for t in acs]
    order = [(i, by, bx) for i, (sh, sv) in enumerate(per_mcu) for by in range(sv) for bx in range(sh)]
    bits, pred = _Bits(), [0] * nc
    segs, mcu = [], 0
    for r in range(rows):
        for cidx in range(cols):
            if restart_mcus and mcu and mcu % restart_mcus == 0:
                bits.flush()
                segs.append(bytes(bits.out))
                bits, pred = _Bits(), [0] * nc
            for i, by, bx in order:
                dcc, acc = dccs[ids[i][1]], accs[ids[i][2]]
                z = planes[i][r * per_mcu[i][1] + by, cidx * per_mcu[i][0] + bx]
                d = int(z[0]) - pred[i]
                pred[i] = int(z[0])
                s = _category(d)
                bits.put(*dcc[s])
                if s:
                    bits.put(d if d > 0 else d - 1, s)
                # the block's AC bits gathered in (bv, bn), one put per block
                zl = z.tolist()
                prev, bv, bn = 0, 0, 0
                for k in range(1, 64):
                    v = zl[k]
                    if v == 0:
                        continue
                    run = k - prev - 1
                    prev = k
                    while run > 15:
                        code, n = acc[0xF0]
                        bv, bn = (bv << n) | code, bn + n
                        run -= 16
                    s = abs(v).bit_length()
                    code, n = acc[(run << 4) | s]
                    bv = (((bv << n) | code) << s) | ((v if v > 0 else v - 1) & ((1 << s) - 1))
                    bn += n + s
                if prev < 63:
                    code, n = acc[0x00]
                    bv, bn = (bv << n) | code, bn + n
                bits.put(bv, bn)
            mcu += 1
    bits.flush()
    segs.append(bytes(bits.out))

    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body

    out = bytearray(b"\xff\xd8")
    if adobe is not None:
        out += seg(0xEE, b"Adobe" + (100).to_bytes(2, "big") + bytes(4) + bytes([adobe]))
    out += seg(0xDB, b"".join(bytes([k]) + bytes(t[ZIGZAG].astype(np.uint8).tolist()) for k, t in enumerate(qts)))
    out += seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc]) +
               b"".join(bytes([i + 1, samp[i][0] << 4 | samp[i][1], ids[i][0]]) for i in range(nc)))
    out += seg(0xC4, b"".join(bytes([k]) + bytes(t[0]) + bytes(t[1]) for k, t in enumerate(dcs)) +
               b"".join(bytes([0x10 | k]) + bytes(t[0]) + bytes(t[1]) for k, t in enumerate(acs)))
    if restart_mcus:
        out += seg(0xDD, restart_mcus.to_bytes(2, "big"))
    out += seg(0xDA, bytes([nc]) + b"".join(bytes([i + 1, ids[i][1] << 4 | ids[i][2]]) for i in range(nc)) +
               bytes([0, 63, 0]))
    for i, s in enumerate(segs):
        if i:
            out += bytes([0xFF, 0xD0 + (i - 1) % 8])
        out += s
    out += b"\xff\xd9"
    return bytes(out)


# Lossless difference categories 0..16, all 5-bit codes.
LOSSLESS_DC = ([0, 0, 0, 0, 17, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], list(range(17)))


def encode_lossless(pixels, psv=1, pt=0, restart_rows=0, table=LOSSLESS_DC, markers=b""):
    """pixels: (H, W) or (H, W, 3) uint8 -> lossless Huffman-coded JPEG
    (SOF3, 8-bit, 1x1 sampling, one interleaved scan; T.81 H.1): predictor
    `psv` (1..7), point transform `pt`, a restart interval of `restart_rows`
    rows of MCUs, `markers` (e.g. an APP segment) after SOI."""
    a = pixels if pixels.ndim == 3 else pixels[:, :, None]
    h, w, nc = a.shape
    x = a.astype(np.int64) >> pt
    codes = _codes(table)
    segs, bits = [], _Bits()
    r0 = 0
    for r in range(h):
        if restart_rows and r and r % restart_rows == 0:
            bits.flush()
            segs.append(bytes(bits.out))
            bits, r0 = _Bits(), r
        for c in range(w):
            for i in range(nc):
                if r == r0:
                    px = (1 << (8 - pt - 1)) if c == 0 else x[r, c - 1, i]
                elif c == 0:
                    px = x[r - 1, c, i]
                else:
                    ra, rb, rc = x[r, c - 1, i], x[r - 1, c, i], x[r - 1, c - 1, i]
                    px = {1: ra, 2: rb, 3: rc, 4: ra + rb - rc, 5: ra + ((rb - rc) >> 1), 6: rb + ((ra - rc) >> 1),
                          7: (ra + rb) >> 1}[psv]
                d = (int(x[r, c, i]) - int(px)) & 0xFFFF
                d = d - 0x10000 if d >= 0x8000 else d
                s = 0 if d == 0 else 16 if d == -32768 else abs(d).bit_length()
                bits.put(*codes[s])
                if 0 < s < 16:
                    bits.put(d if d > 0 else d - 1, s)
    bits.flush()
    segs.append(bytes(bits.out))

    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body

    out = bytearray(b"\xff\xd8") + markers
    out += seg(0xC3, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc]) +
               b"".join(bytes([i + 1, 0x11, 0]) for i in range(nc)))
    out += seg(0xC4, bytes([0x00]) + bytes(table[0]) + bytes(table[1]))
    if restart_rows:
        out += seg(0xDD, (restart_rows * w).to_bytes(2, "big"))
    out += seg(0xDA, bytes([nc]) + b"".join(bytes([i + 1, 0x00]) for i in range(nc)) + bytes([psv, 0, pt]))
    for i, s in enumerate(segs):
        if i:
            out += bytes([0xFF, 0xD0 + (i - 1) % 8])
        out += s
    out += b"\xff\xd9"
    return bytes(out)
