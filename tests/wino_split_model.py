"""Exact numpy model of the split-bf16 ("bf16x2") Winograd path (csrc/winograd.hip: wino_pack_bf16x2, wino_gemm_bf16x2_kernel).

A value travels as one 32-bit word: hi = bf16(x) in the low half, mid = bf16(x - hi) in the high half, both round-to-nearest-even.
The GEMM adds three bf16 x bf16 products per k (um*vh + uh*vm + uh*vh, every product exact in f32) and drops um*vm.  Everything here is
numpy on the CPU; tests/test_wino_split_model_cpu.py pins it, tests/test_gpu_wino_bf16x2.py holds the kernels to it.
"""
from __future__ import annotations

import numpy as np

U24 = 2.0 ** -24                                  # unit roundoff of f32


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u) for f32 accumulation."""
    return n * U24 / (1.0 - n * U24)


def _rne_bf16_bits(bits):
    """f32 bit patterns (uint32, finite values) -> the upper 16 bits rounded to nearest even, as uint32.  The carry of a mantissa of
    all ones runs into the exponent: the next binade, or 0x7F80 = Inf from 0x7F7F8000 up."""
    bits = bits.astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint32)


def split(x):
    """x (f32, finite) -> (hi, mid, word): hi = RNE bf16 of x, mid = RNE bf16 of r = x - hi (r is exact in f32: it is a multiple of x's
    last bit and at most half a bf16 ulp of x), both returned as f32 arrays; word = hi's 16 bits | mid's 16 bits << 16 (uint32)."""
    x = np.ascontiguousarray(x, np.float32)
    hb = _rne_bf16_bits(x.view(np.uint32))
    hi = (hb << 16).view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (x - hi).astype(np.float32)
    mb = _rne_bf16_bits(r.view(np.uint32))
    mid = (mb << 16).view(np.float32)
    return hi, mid, (hb | (mb << 16)).astype(np.uint32)


def unpack(word):
    """packed words (uint32) -> (hi, mid) as f32"""
    word = np.ascontiguousarray(word, np.uint32)
    return (word << 16).view(np.float32), (word & np.uint32(0xFFFF0000)).view(np.float32)


def is_bf16_normal(h):
    """True where the bf16 value held in the f32 `h` is a normal number (not zero, subnormal, Inf or NaN)."""
    e = (np.ascontiguousarray(h, np.float32).view(np.uint32) >> 23) & 0xFF
    return (e != 0) & (e != 0xFF)


def gemm_halves(vh, vm, uh, um, terms=("mh", "hm", "hh")):
    """[..., rows, K] x [..., N, K] halves -> (M, S) in fp64.  terms, named u-half then v-half: "mh" = um*vh, "hm" = uh*vm, "hh" = uh*vh
    (the kernel's three MFMAs, in its order) and "mm" = um*vm, which the kernel drops.  S is the sum of the terms' magnitudes."""
    vh, vm, uh, um = (np.asarray(a, np.float64) for a in (vh, vm, uh, um))
    pick = {"mh": (um, vh), "hm": (uh, vm), "hh": (uh, vh), "mm": (um, vm)}
    M = S = 0.0
    for t in terms:
        u, v = pick[t]
        M = M + v @ np.swapaxes(u, -1, -2)
        S = S + np.abs(v) @ np.swapaxes(np.abs(u), -1, -2)
    return M, S


def gemm_model(V, U):
    """V [..., rows, K], U [..., N, K] (f32) -> M = sum_k (um*vh + uh*vm + uh*vh) and S = sum_k (|um*vh| + |uh*vm| + |uh*vh|), fp64."""
    vh, vm, _ = split(V)
    uh, um, _ = split(U)
    return gemm_halves(vh, vm, uh, um)


# F(4x4, 3x3), interpolation points 0, +-1, +-2, inf (Lavin & Gray 2016), as csrc/winograd.hip writes them
BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
               [0, 4, 0, -5, 0, 1]], np.float64)
G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
             np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)


def filter_transform(w):
    """w [Cout, Cin, 3, 3] -> U [36, Cout, Cin] = G g G^T in fp64, cast to f32 (what the loader stores), f = 6 i + j"""
    u = np.einsum("ia,ocab,jb->ijoc", G, np.asarray(w, np.float64), G)
    return u.reshape(36, w.shape[0], w.shape[1]).astype(np.float32)


def input_transform(x):
    """x [B, C, H, W] -> V [36, B*TY*TX, C] = B^T d B of the zero-padded 6x6 patches (uniform tiling, overhanging tiles), rounded to f32.
    The input is rounded to f32 first: that is what the layer reads."""
    x = np.asarray(x, np.float32).astype(np.float64)
    B, C, H, W = x.shape
    TY, TX = (H + 3) // 4, (W + 3) // 4
    xp = np.zeros((B, C, 4 * TY + 2, 4 * TX + 2))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    s = xp.strides
    d = np.lib.stride_tricks.as_strided(xp, (B, C, TY, TX, 6, 6), (s[0], s[1], 4 * s[2], 4 * s[3], s[2], s[3]))
    v = np.einsum("ia,bcyxaj,lj->ilbyxc", BT, d, BT)
    return v.reshape(36, B * TY * TX, C).astype(np.float32), (B, TY, TX)


def conv_model(x, w, b=None):
    """3x3 stride-1 pad-1 convolution as the split-bf16 Winograd layer computes it: x [B, Cin, H, W], w [Cout, Cin, 3, 3], b [Cout] or
    None -> [B, Cout, H, W] in fp64.  U and V rounded to f32 and split, the GEMM is gemm_model, the output transform is fp64."""
    H, W = x.shape[2], x.shape[3]
    V, (B, TY, TX) = input_transform(x)
    M, _ = gemm_model(V, filter_transform(w))                                          # [36, tiles, Cout]
    m = M.reshape(6, 6, B, TY, TX, -1)
    y = np.einsum("pi,ijbyxo,qj->boypxq", AT, m, AT).reshape(B, -1, 4 * TY, 4 * TX)[:, :, :H, :W]
    if b is not None:
        y = y + np.asarray(b, np.float64)[None, :, None, None]
    return np.ascontiguousarray(y)


def conv_fp64(x, w, b=None):
    """the same convolution directly in fp64"""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64)
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    y = np.zeros((B, w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            y += np.einsum("bcyx,oc->boyx", xp[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
    if b is not None:
        y += np.asarray(b, np.float64)[None, :, None, None]
    return y


# ---------------------------------------------------------------------------------------------------------------- crafted operands
def crafted_words():
    """f32 bit patterns that sit on the format's edges: +-0; ties at the hi boundary (to even both ways); the carry of a full mantissa
    into the next binade; negative mid; mid ties; the smallest values whose mid is still a bf16 normal."""
    w = [0x00000000, 0x80000000,
         0x3F808000, 0x3F818000,              # 1 + 2^-8 (tie: hi stays at the even 1.0), 1 + 3 * 2^-8 (tie: hi goes up to the even 1 + 2^-6)
         0xBF808000, 0xBF818000,
         0x3F7FFFFF,                          # 1 - 2^-24: hi carries into the next binade (1.0), mid = -2^-24
         0x3F80C000, 0x3F80FFFF, 0x3F808001,  # just above a tie: hi rounds up, mid is negative
         0x3F800101, 0x3F800103,              # ties of mid: r = 2^-15 (1 + 2^-8) stays at the even 2^-15, 2^-15 (1 + 3 * 2^-8) goes up
         0x3F800080, 0x3F800180, 0x3F807FFF, 0x3F800001, 0x3F80FF80,
         0x7F7F7FFF,                          # the largest value whose hi is finite
         0x0C000001, 0x8C000001,              # +-2^-103 (1 + 2^-23): mid = +-2^-126, the smallest bf16 normal
         0x0C800001, 0x00800000, 0x00810000,  # hi at the bottom of the normal range (mid = 0)
         0x40490FDB, 0xC0490FDB, 0x3EAAAAAB, 0x42F6E979]
    return np.array(w, np.uint32)


def random_words(rng, n):
    """n seeded random f32 bit patterns, finite with |x| < 2^127, whose hi and mid are each zero or a bf16 normal"""
    out = np.empty(0, np.uint32)
    while out.size < n:
        w = rng.integers(0, 1 << 32, 2 * n, dtype=np.uint64).astype(np.uint32)
        e = (w >> 23) & 0xFF
        w = w[e < 0xFE]                                                   # finite, |x| < 2^127
        hi, mid, _ = split(w.view(np.float32))
        ok = (is_bf16_normal(hi) | (hi == 0)) & (is_bf16_normal(mid) | (mid == 0))
        out = np.concatenate([out, w[ok]])
    return out[:n]


def quantize(x, bits):
    """f32 values rounded to `bits` significant bits (round to nearest even on the bit pattern)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    drop = 24 - bits
    if drop > 0:
        b = ((b + ((1 << (drop - 1)) - 1) + ((b >> drop) & 1)) >> drop) << drop
    return b.astype(np.uint32).view(np.float32)


# C.2's operand classes: significand bits of V and of the weight value
ONE_HOT_CLASSES = {"a": (16, 8), "b": (8, 16), "c": (12, 12)}


def one_hot_kk(K, N):
    """kk[f, n]: the single k at which U[f][n][:] is non-zero.  (5 f + 3 n) mod K: for a fixed f, n = 0 .. N-1 walks the residues in steps
    of 3 — coprime to every K = 32 m — so with N >= K every k (hence every position mod 8 and mod 32) is hit in EVERY frequency; for N < K
    the 36 frequencies shift the window by 5 each, and the union over f still covers 0 .. K-1 (asserted by the tests); neighbouring
    frequencies always differ."""
    f = np.arange(36)[:, None]
    n = np.arange(N)[None, :]
    return (5 * f + 3 * n) % K


def one_hot_operands(rng, rows, K, N, cls, w_per_freq=True):
    """V [rows, K] random with cls's significand width, wv [36, N] weight values (a different one per frequency and column), kk [36, N].
    Values are O(1) with signs; none is zero."""
    vb, wb = ONE_HOT_CLASSES[cls]
    V = quantize((rng.uniform(0.5, 2.0, (rows, K)) * rng.choice([-1.0, 1.0], (rows, K))).astype(np.float32), vb)
    wv = quantize((rng.uniform(0.5, 2.0, (36, N)) * rng.choice([-1.0, 1.0], (36, N))).astype(np.float32), wb)
    return V, wv, one_hot_kk(K, N)


def one_hot_expected(v, w):
    """the three-term product of one V value and one weight value, exact: um*vh + uh*vm + uh*vh = v*w - vm*wm when both split exactly
    (<= 16 significant bits).  fp64 holds it exactly (every term has <= 16 bits, exponents within 2^-18 of each other)."""
    vh, vm, _ = split(v)
    uh, um, _ = split(w)
    vh, vm, uh, um = (a.astype(np.float64) for a in (vh, vm, uh, um))
    return um * vh + uh * vm + uh * vh


def dense_operands(rng, rows, K, N, kind):
    """C.3's operands.  "normal": V ~ N(0,1), U ~ N(0,1)/sqrt(K).  "positive": every value positive with a large positive mid — hi in
    [1, 1.25) * 2^e and mid in [0.5, 1) of half a bf16 ulp — so that a lost cross term is a COHERENT error of about 2^-9.6 of S.
    In both sets a value whose mid would be zero gets its last bit set: every half is a bf16 normal."""
    if kind == "normal":
        V = rng.standard_normal((rows, K)).astype(np.float32)
        U = (rng.standard_normal((36, N, K)) / np.sqrt(K)).astype(np.float32)
    else:
        def pos(shape, scale):
            hi = quantize((rng.uniform(1.0, 1.25, shape) * scale).astype(np.float32), 8)
            e = np.floor(np.log2(hi.astype(np.float64)))
            return (hi.astype(np.float64) + rng.uniform(0.5, 0.98, shape) * 2.0 ** (e - 8)).astype(np.float32)
        V = pos((rows, K), 1.0)
        U = pos((36, N, K), 1.0 / np.sqrt(K))

    def fix(a):
        _, mid, _ = split(a)
        b = a.view(np.uint32).copy()
        b[mid == 0] |= 1
        return b.view(np.float32)
    return fix(V), fix(U)


# ------------------------------------------------------------------------------------------------- plane layouts of the GEMM stage
def uniform_planes(tiles):
    """uniform tiling: 36 planes of wino_rows(tiles) = tiles rounded up to 256 rows -> [(first row, real rows, padded rows, frequency)]"""
    ntp = (tiles + 255) // 256 * 256
    return [(f * ntp, tiles, ntp, f) for f in range(36)]


def mixed_planes(B, H, W):
    """mixed F(4x4) / F(2x2) tiling (docs/kernels.md 3.1j): classes (rows F4 | F2) x (columns F4 | F2) one after the other, plane-major
    inside a class, every plane padded to whole 128-row tiles; plane (i, j) of an F(2) direction uses frequency {0, 1, 2, 5}[i]."""
    TY, TX = (H + 3) // 4, (W + 3) // 4
    my, mx = int(H % 4 in (1, 2)), int(W % 4 in (1, 2))
    n = [(TY - my) * (TX - mx), (TY - my) * mx, my * (TX - mx), my * mx]
    f2map = (0, 1, 2, 5)
    out, row = [], 0
    for c in range(4):
        nfr, nfc = (4 if c & 2 else 6), (4 if c & 1 else 6)
        rows = (B * n[c] + 127) // 128 * 128
        for i in range(nfr):
            for j in range(nfc):
                fi = f2map[i] if c & 2 else i
                fj = f2map[j] if c & 1 else j
                if rows:
                    out.append((row, B * n[c], rows, 6 * fi + fj))
                row += rows
    return out
