"""The Huffman coder of the JPEG encoder as a numpy model of its PARALLEL decomposition (include/facehip.h "JPEG out", csrc/jpeg_huff.hip):
every block coded on its own — the DC predictor taken from the neighbouring block, not from a running value —, a prefix sum of the
blocks' bits, the codes placed at their offsets, the last byte padded with ones, the 0xFF bytes counted and prefix-summed, and
header + stuffed stream + EOI.  Written down independently of csrc/image_io.cpp (the Annex K tables are restated here); held to
fh_jpeg_scan_bits and fh_jpeg_write by tests/test_jpeg_huff_cpu.py, and what the device passes are debugged against.  Plus the crafted
coefficient planes and the ctypes helpers the coder's tests share (tests/test_gpu_jpeg_huff.py)."""
import ctypes as C

import numpy as np

from tests import jpeg_enc_model as m

FH_ERR_ARG = -1
KS = [1, 15, 16, 17, 32, 33, 48, 49, 62, 63]                               # zigzag positions: ZRL counts 0..3, and no EOB at 63

# ITU T.81 Annex K.3: the number of codes of each length 1..16 and the symbols, DC / AC, luminance / chrominance
DC_VALS = list(range(12))
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa]
STD = [([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], DC_VALS), ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], DC_VALS),
       ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], AC_LUMA_VALS), ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], AC_CHROMA_VALS)]


def _tables():
    """[DC luma, DC chroma, AC luma, AC chroma] as {symbol: (code, length)}: T.81 Annex C."""
    out = []
    for bits, vals in STD:
        t, code, k = {}, 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                t[vals[k]] = (code, length)
                code += 1
                k += 1
            code <<= 1
        out.append(t)
    return out


TABLES = _tables()


# ------------------------------------------------------------------------------------------ the rule, block by block
def scan(desc):
    """The blocks of the interleaved scan, in order: [(component, block row, block column, (component, row, column) of the block whose DC
    predicts this one's, or None)].  The predictor is a NEIGHBOUR: the block in front of it inside the MCU, else the component's last block
    of the MCU in front, else nothing."""
    comps = [desc.comp[i] for i in range(desc.ncomp)]
    mcux, mcuy = comps[0].wblocks // comps[0].h, comps[0].hblocks // comps[0].v
    out = []
    for mcu in range(mcux * mcuy):
        my, mx = divmod(mcu, mcux)
        for ci, c in enumerate(comps):
            for q in range(c.h * c.v):
                def at(m_, q_):
                    y, x = divmod(q_, c.h)
                    return ci, (m_ // mcux) * c.v + y, (m_ % mcux) * c.h + x
                prev = at(mcu, q - 1) if q > 0 else at(mcu - 1, c.h * c.v - 1) if mcu > 0 else None
                out.append(at(mcu, q) + (prev,))
    return out


def _size(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, n):
    v = int(v)
    return (v if v >= 0 else v - 1) & ((1 << n) - 1)


def block_codes(zz, pred, ci):
    """The 64 (code, length) pairs of one block, one per zigzag position, each formed from the block's non-zero mask alone (what a lane of
    the device's wave does); None for a block the baseline tables cannot code."""
    dc, ac = TABLES[1 if ci else 0], TABLES[3 if ci else 2]
    out = [(0, 0)] * 64
    diff = int(zz[0]) - int(pred)
    n = _size(diff)
    if n > 11:
        return None
    code, length = dc[n]
    out[0] = ((code << n) | _value_bits(diff, n), length + n)
    nz = [k for k in range(1, 64) if zz[k] != 0]
    for k in nz:
        below = [j for j in nz if j < k]
        run = k - (below[-1] if below else 0) - 1
        n = _size(zz[k])
        if n > 10:
            return None
        code, length = 0, 0
        for _ in range(run >> 4):
            code, length = (code << ac[0xF0][1]) | ac[0xF0][0], length + ac[0xF0][1]
        sc, sl = ac[((run & 15) << 4) | n]
        out[k] = ((((code << sl) | sc) << n) | _value_bits(zz[k], n), length + sl + n)
    if zz[63] == 0:
        out[63] = ac[0x00]
    return out


def image_codes(desc, coef):
    """[64 (code, length) pairs] per block of the scan; None when a block has no code."""
    coef = np.asarray(coef)

    def block(ci, by, bx):
        c = desc.comp[ci]
        at = int(c.coef_off) + (by * c.wblocks + bx) * 64
        return coef[at: at + 64]
    out = []
    for ci, by, bx, prev in scan(desc):
        codes = block_codes(block(ci, by, bx)[m.ZIGZAG], 0 if prev is None else block(*prev)[0], ci)
        if codes is None:
            return None
        out.append(codes)
    return out


def scan_bits(desc, coef):
    """The bits of every block of the scan (fh_jpeg_scan_bits), or None."""
    codes = image_codes(desc, coef)
    return None if codes is None else np.array([sum(length for _, length in blk) for blk in codes], np.uint32)


def stream(desc, coef):
    """The unstuffed entropy-coded bytes: prefix sum of the lengths, every code OR-ed in at its offset, the last byte padded with ones."""
    codes = [cl for blk in image_codes(desc, coef) for cl in blk]
    lengths = np.array([length for _, length in codes], np.int64)
    offs = np.cumsum(lengths) - lengths                                      # exclusive
    total = int(lengths.sum())
    nbytes = (total + 7) // 8
    acc = 0
    for (code, length), off in zip(codes, offs):
        acc |= code << (nbytes * 8 - int(off) - length)
    acc |= (1 << (nbytes * 8 - total)) - 1                                   # the pad: ones
    return np.frombuffer(acc.to_bytes(nbytes, "big"), np.uint8)


def stuff(raw):
    """A zero behind every 0xFF: byte j goes to j + the 0xFF bytes in front of it."""
    ff = (raw == 0xFF).astype(np.int64)
    at = np.arange(len(raw)) + np.cumsum(ff) - ff
    out = np.zeros(len(raw) + int(ff.sum()), np.uint8)
    out[at] = raw
    return out


def file_bytes(desc, coef):
    """header (fh_jpeg_write_header's) + the stuffed stream + EOI."""
    rc, n, hdr = c_header(desc)
    assert rc == 0
    return hdr[:n].tobytes() + stuff(stream(desc, coef)).tobytes() + b"\xff\xd9"


# ------------------------------------------------------------------------------------------ crafted coefficient planes
def _plane(desc):
    return np.zeros(int(desc.coef_count), np.int16)


def _blocks(desc, coef, ci=0):
    c = desc.comp[ci]
    return coef[int(c.coef_off): int(c.coef_off) + c.wblocks * c.hblocks * 64].reshape(c.hblocks * c.wblocks, 64)


def _extreme(blk, dc):
    """All 63 AC = +-1023 (positive at odd zigzag positions, so the block ends in ten one-bits) behind DC = dc."""
    blk[m.ZIGZAG[1:]] = [1023 if k % 2 else -1023 for k in range(1, 64)]
    blk[0] = dc


def crafted():
    """[(name, descriptor, int16 coefficients)]: the code paths a picture rarely reaches, every one codable."""
    out = []
    d = m.enc_desc(64, 64, "grey", 90); out.append(("zero_grey", d, _plane(d)))          # 64 blocks of 6 bits: 48 bytes, no pad
    d = m.enc_desc(48, 32, "420", 90); out.append(("zero_420", d, _plane(d)))
    for layout, (w, h) in (("grey", (80, 8)), ("420", (80, 32))):                        # one value per block at each of KS
        d = m.enc_desc(w, h, layout, 90); coef = _plane(d)
        for ci in range(d.ncomp):
            for b, blk in enumerate(_blocks(d, coef, ci)):
                blk[m.ZIGZAG[KS[(b + ci) % len(KS)]]] = (5, -3, 1, -1, 1023, -1023, 77)[(b + 2 * ci) % 7]
                blk[0] = (b * 37 + ci * 11) % 200 - 100
        out.append((f"single_{layout}", d, coef))
    d = m.enc_desc(64, 16, "grey", 90); coef = _plane(d)                                  # the longest blocks, DC steps +2047 / -2047
    for b, blk in enumerate(_blocks(d, coef)):
        _extreme(blk, 2047 * ((b + 1) % 2))
    out.append(("extreme_grey", d, coef))
    d = m.enc_desc(32, 16, "420", 90); coef = _plane(d)
    for ci in range(3):
        for b, blk in enumerate(_blocks(d, coef, ci)):
            _extreme(blk, (2047, -2047, 2047)[ci] * ((b + 1) % 2))
    out.append(("extreme_420", d, coef))
    d = m.enc_desc(128, 8, "grey", 90); coef = _plane(d)                                  # DC 0, 2047, 4094, ...: the difference stays +2047
    for b, blk in enumerate(_blocks(d, coef)):
        blk[0] = 2047 * b
    out.append(("ramp_grey", d, coef))
    d = m.enc_desc(16, 64, "420", 90); coef = _plane(d)                                   # (one MCU per row: luma's scan order is its raster order)
    for ci in range(3):
        for b, blk in enumerate(_blocks(d, coef, ci)):
            blk[0] = (2047, -2047, 2047)[ci] * b
    out.append(("ramp_420", d, coef))
    for layout, (w, h) in (("grey", (64, 8)), ("420", (32, 32))):                        # FFFE + ten ones + FFFE: 25 one-bits in a row
        d = m.enc_desc(w, h, layout, 90); coef = _plane(d)
        for b, blk in enumerate(_blocks(d, coef)):
            blk[m.ZIGZAG[16]] = blk[m.ZIGZAG[32]] = 1023
            blk[0] = (0, 1, 3, 7, 20, 100, 300, 1000)[b % 8]                             # DC sizes 0..10: the run starts at every bit phase
        out.append((f"ones_{layout}", d, coef))
    return out


def uncodable():
    """[(name, descriptor, coefficients)]: one coefficient each that the baseline tables cannot code."""
    out = []

    def grey(name, edit):
        d = m.enc_desc(24, 8, "grey", 90); coef = _plane(d)
        edit(_blocks(d, coef))
        out.append((name, d, coef))
    grey("dc+2048", lambda b: b[0].__setitem__(0, 2048))
    grey("dc-2048", lambda b: b[1].__setitem__(0, -2048))
    grey("dc_full_swing", lambda b: (b[1].__setitem__(0, -32768), b[2].__setitem__(0, 32767)))
    grey("ac+1024", lambda b: b[2].__setitem__(m.ZIGZAG[5], 1024))
    grey("ac-1024", lambda b: b[0].__setitem__(m.ZIGZAG[63], -1024))
    grey("ac-32768", lambda b: b[1].__setitem__(m.ZIGZAG[1], -32768))
    d = m.enc_desc(16, 16, "420", 90); coef = _plane(d)
    _blocks(d, coef, 2)[0][m.ZIGZAG[40]] = 32767
    out.append(("chroma_ac_32767", d, coef))
    return out


# ------------------------------------------------------------------------------------------ the C ABI through ctypes
def c_header(desc, cap=1024, guard=0):
    """fh_jpeg_write_header into a buffer of cap + guard bytes pre-filled with 0xA5: (rc, written, buffer)."""
    L, _ = m._fa()
    out = np.full(max(cap + guard, 1), 0xA5, np.uint8)
    written = C.c_size_t(12345)
    rc = L.fh_jpeg_write_header(C.byref(desc), out.ctypes.data, cap, C.byref(written))
    return rc, int(written.value), out


def blocks_of(desc):
    return sum(desc.comp[i].wblocks * desc.comp[i].hblocks for i in range(desc.ncomp))


def c_scan_bits(desc, coef, cap=None, guard=0):
    """fh_jpeg_scan_bits into an array of cap (default: the scan's blocks) + guard entries pre-filled with 0xA5A5A5A5: (rc, array)."""
    L, _ = m._fa()
    cap = blocks_of(desc) if cap is None else cap
    bits = np.full(max(cap + guard, 1), 0xA5A5A5A5, np.uint32)
    rc = L.fh_jpeg_scan_bits(C.byref(desc), np.ascontiguousarray(coef).ctypes.data, bits.ctypes.data, cap)
    return rc, bits
