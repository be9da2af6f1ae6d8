"""Locality / isolation helpers: which inputs may influence which outputs, and buffers that show when something else did.

The property (tests/test_gpu_locality.py): change an input only at a set Q of elements, to NaN / +-Inf.  Outside the allowed set A(Q) —
the outputs whose receptive field holds an element of Q — the output must equal the clean run BIT FOR BIT.  A(Q) per convolution form is a
Chebyshev radius R in output coordinates around each poisoned pixel (its coordinates divided by the stride first); the radii come from
the algorithms (tests/test_locality_model_cpu.py derives them from numpy emulations), not from the kernels:

    direct 3x3 : 1      1x1 : 0      fused F(2x2,3x3) : 2      F(4x4,3x3) incl. the mixed F(4) / F(2) tiling : 4

Everything here is numpy; only GuardedBuffer.upload / download touch the device (torch is imported there).
"""
from __future__ import annotations

import numpy as np

R_DIRECT3, R_1X1, R_WINO2, R_WINO4 = 1, 0, 2, 4

NAN_BITS, PINF_BITS, NINF_BITS = 0x7FC00000, 0x7F800000, 0xFF800000
PATTERNS = (("nan", NAN_BITS), ("+inf", PINF_BITS), ("-inf", NINF_BITS))
CANARY_BITS = 0xA5C3961E                       # output guards: a finite, unlikely fp32 (-3.39e-16) — any store into a guard changes it

GUARD_MIN = 64 * 1024


def bits_to_f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


# ------------------------------------------------------------------------------------------------ allowed sets
def allowed_mask(shape, Q, stride, R):
    """bool [B, Ho, Wo]: the output pixels a poisoned input pixel may reach.  shape = (B, Ho, Wo) of the OUTPUT; Q = iterable of input
    pixels (b, y, x); each is divided by `stride` and exempts the Chebyshev ball of radius R around it, clipped to its own image.
    Asserts the exemption cap: at most (2R+1)^2 output pixels per poisoned input pixel."""
    B, Ho, Wo = shape
    m = np.zeros((B, Ho, Wo), bool)
    Q = list(Q)
    for (b, y, x) in Q:
        assert 0 <= b < B, (b, B)
        oy, ox = y // stride, x // stride
        one = np.zeros((Ho, Wo), bool)
        one[max(0, oy - R):min(Ho, oy + R + 1), max(0, ox - R):min(Wo, ox + R + 1)] = True
        assert one.sum() <= (2 * R + 1) ** 2
        m[b] |= one
    assert m.sum() <= len(Q) * (2 * R + 1) ** 2, (int(m.sum()), len(Q), R)
    return m


def propagate_conv_mask(mask, k, stride):
    """The EXACT receptive-field image of a pixel mask through one k x k convolution (k = 1 or 3, padding k // 2): output pixel (oy, ox)
    is set iff one of its in-image taps (oy * stride + dy, ox * stride + dx), |dy|, |dx| <= k // 2, is set.  mask: bool [B, H, W]."""
    B, H, W = mask.shape
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    padded = np.zeros((B, H + 2 * p, W + 2 * p), bool)
    padded[:, p:p + H, p:p + W] = mask
    out = np.zeros((B, Ho, Wo), bool)
    for dy in range(k):
        for dx in range(k):
            out |= padded[:, dy:dy + (Ho - 1) * stride + 1:stride, dx:dx + (Wo - 1) * stride + 1:stride]
    return out


def propagate_graph_mask(g, mask):
    """Pixel mask [B, H, W] of the graph input -> {output name: mask [B, Ho, Wo]} through an oracle.onnx_min graph of the direct-form
    vocabulary: Conv (1x1 / 3x3, any stride and group: a poisoned channel of a pixel is taken to poison the whole pixel), element-wise ops
    (pass), Add (union), x2 Upsample / Resize (repeat), and the channels-last Transpose + Reshape tail (pass)."""
    env = {g.inputs[0][0]: mask}
    for n in g.nodes:
        ins = [env[k] for k in n.inputs if k in env]
        if n.op == "Conv":
            k = n.attrs["kernel_shape"][0]
            s = n.attrs.get("strides", [1, 1])[0]
            assert k in (1, 3) and n.attrs.get("pads", [0] * 4)[0] == k // 2, n.attrs
            y = propagate_conv_mask(ins[0], k, s)
        elif n.op == "Add" and len(ins) == 2:
            y = ins[0] | ins[1]
        elif n.op in ("Upsample", "Resize"):
            y = ins[0].repeat(2, axis=1).repeat(2, axis=2)
        elif n.op in ("Relu", "PRelu", "Sigmoid", "BatchNormalization", "Identity", "Dropout", "Mul", "Sub", "Div", "Add",
                      "Transpose", "Reshape"):
            if len(ins) != 1:                                    # element-wise op of two tensors (only Add is handled, above)
                raise NotImplementedError(f"{n.op} of {len(ins)} tensors")
            y = ins[0]
        else:
            raise NotImplementedError(n.op)
        env[n.outputs[0]] = y
    return {name: env[name] for name, _ in g.outputs}


# ------------------------------------------------------------------------------------------------ plants
def plant_positions(B, H, W):
    """The fixed within-image plant positions [(tag, b, y, x)], duplicates removed (small maps / B = 1 fold several onto one pixel):
    pixel (0,0) of image 0 and of a middle image, the last pixel of the last image, the last pixel of image i and the first of image
    i + 1 (a batch boundary), one interior pixel, one pixel on each border."""
    mid = B // 2
    i = max(0, min(B - 2, B // 3))                       # the batch boundary i | i + 1
    cand = [("first", 0, 0, 0), ("mid-first", mid, 0, 0), ("last", B - 1, H - 1, W - 1)]
    if B > 1:
        cand += [("boundary-last", i, H - 1, W - 1), ("boundary-first", i + 1, 0, 0)]
    bi = min(B - 1, 1) if B > 1 else 0                   # interior / border pixels: another image where there is one
    cand += [("interior", bi, H // 2, W // 2), ("top", bi, 0, W // 2), ("bottom", bi, H - 1, W // 3),
             ("left", mid, H // 2, 0), ("right", mid, H // 3, W - 1)]
    seen, out = set(), []
    for tag, b, y, x in cand:
        if (b, y, x) not in seen:
            seen.add((b, y, x))
            out.append((tag, b, y, x))
    return out


def plant_list(B, H, W, C):
    """-> [(tag, b, y, x, c, pattern name, pattern bits)]: every position of plant_positions in channel 0 and in the last channel, the
    three patterns NaN / +Inf / -Inf dealt round-robin over that list (fixed, not random)."""
    out = []
    k = 0
    for tag, b, y, x in plant_positions(B, H, W):
        for c in sorted({0, C - 1}):
            name, bits = PATTERNS[k % 3]
            out.append((tag, b, y, x, c, name, bits))
            k += 1
    return out


def plant_groups(B, H, W, C):
    """plant_list split by pattern: three groups, each planted in a dirty run of its own (fewer plants per run: a leak of one plant cannot
    hide in another plant's allowed set as easily).  Every group is non-empty for every shape (>= 3 positions x >= 1 channel)."""
    pl = plant_list(B, H, W, C)
    groups = [[p for p in pl if p[5] == name] for name, _ in PATTERNS]
    assert all(groups)
    return groups


def apply_plants(x_nhwc, plants):
    """Copy of x [B, H, W, C] float32 with the plants' bit patterns written in."""
    y = x_nhwc.copy()
    v = y.view(np.uint32)
    for _, b, yy, xx, c, _, bits in plants:
        v[b, yy, xx, c] = bits
    return y


def aggressor_victim_sets(B):
    """Victim images of the aggressor leg, one list per dirty run: image 0, the last image and every third in between — at least a third
    of the batch.  B = 2 would leave no aggressor that way: two runs, each image the victim once."""
    assert B >= 2
    if B == 2:
        return [[0], [1]]
    v = sorted(set(range(0, B, 3)) | {0, B - 1})
    assert 3 * len(v) >= B and len(v) < B
    return [v]


def hostile_images(shape, C_live, seed):
    """Aggressor images [B, H, W, C] that survive a ReLU behind the first convolution (an all-NaN image does not: max-style ReLU turns it
    into an all-zero map, the value of zero padding): N(0, 8^2) noise in the first C_live lanes, 0 in the others, and +Inf in lane 0 of
    a sparse pixel grid (every 5th row / column: the 3x3 windows of two grid pixels never overlap, so a convolution behind them yields
    +-Inf, not Inf - Inf = NaN) plus the image's last pixel (which may sit one or two rows / columns from a grid pixel: a few outputs
    there can be NaN, and 0 behind a ReLU — harmless, the rest of the grid is what has to survive)."""
    B, H, W, C = shape
    rng = np.random.default_rng(seed)
    out = np.zeros(shape, np.float32)
    out[..., :C_live] = (8.0 * rng.standard_normal((B, H, W, C_live))).astype(np.float32)
    out[:, ::5, ::5, 0] = np.inf
    out[:, H - 1, W - 1, 0] = np.inf
    return out


# ------------------------------------------------------------------------------------------------ comparisons
def assert_images_changed(got_dirty, got_clean, images, what="", need_nonfinite=False):
    """Not vacuous: every image flagged in `images` [B] has an output that differs from the clean run in some bit (something hostile did
    arrive in front of the kernels); need_nonfinite: and holds a non-finite value (the poison survived to the output)."""
    a = np.ascontiguousarray(got_dirty); b = np.ascontiguousarray(got_clean)
    B = a.shape[0]
    au = a.view(np.uint32).reshape(B, -1); bu = b.view(np.uint32).reshape(B, -1)
    for i in np.nonzero(np.asarray(images, bool))[0]:
        assert (au[i] != bu[i]).any(), f"{what}: image {i} was changed in the input but its output is bitwise the clean run's"
        if need_nonfinite:
            assert not np.isfinite(a[i]).all(), f"{what}: image {i}: no non-finite value reached the output"


def assert_bitwise_outside(got_dirty, got_clean, allowed, what=""):
    """got_* [B, Ho, Wo, C] float32 (or anything whose leading dims match `allowed` [B, Ho, Wo] / [B]); outside `allowed` the two must be
    equal as uint32.  Returns (exempted elements, compared elements)."""
    a = np.ascontiguousarray(got_dirty); b = np.ascontiguousarray(got_clean)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, b.shape, a.dtype, b.dtype)
    allowed = np.asarray(allowed, bool)
    assert a.shape[:allowed.ndim] == allowed.shape, (a.shape, allowed.shape)
    per = int(np.prod(a.shape[allowed.ndim:], dtype=np.int64))
    au = a.view(np.uint32).reshape(allowed.shape + (per,)); bu = b.view(np.uint32).reshape(allowed.shape + (per,))
    diff = (au != bu).any(axis=-1) & ~allowed
    if diff.any():
        idx = np.argwhere(diff)
        first = tuple(int(v) for v in idx[0])
        raise AssertionError(f"{what}: {len(idx)} output pixels outside the allowed set differ from the clean run bitwise; first at {first}: "
                             f"dirty {a.reshape(allowed.shape + (per,))[first][:4]} clean {b.reshape(allowed.shape + (per,))[first][:4]}; "
                             f"images touched {sorted(set(int(v[0]) for v in idx))[:8]}")
    return int(allowed.sum()) * per, int((~allowed).sum()) * per


def assert_poison_was_read(got_dirty, Q, in_hw, stride, k, what=""):
    """Not vacuous (layers without activation): every output pixel whose direct-form k x k receptive field holds a poisoned pixel is
    non-finite in every channel.  got_dirty [B, Ho, Wo, C]; Q = [(b, y, x)] on the input grid in_hw = (H, W)."""
    B, Ho, Wo = got_dirty.shape[:3]
    m = np.zeros((B,) + tuple(in_hw), bool)
    for b, y, x in Q:
        m[b, y, x] = True
    need = propagate_conv_mask(m, k, stride)
    assert need.shape == (B, Ho, Wo)
    bad = need & np.isfinite(got_dirty).reshape(B, Ho, Wo, -1).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} outputs inside the receptive field of a plant stayed finite, first {np.argwhere(bad)[0]}"
    return int(need.sum())


# ------------------------------------------------------------------------------------------------ guard-banded buffers
def guard_layout(nbytes, guard=GUARD_MIN):
    """-> (offset of the tensor, total bytes) of one allocation [guard | tensor | guard]: each guard >= 64 KiB and a multiple of 256 B
    (the tensor starts on a 256-byte boundary of a 256-byte-aligned allocation, so 16-byte lane accesses stay aligned); the rear guard is
    stretched so that the allocation ends on a 256-byte boundary too."""
    g = max(GUARD_MIN, (int(guard) + 255) // 256 * 256)
    rear = g + (-(g + nbytes)) % 256
    assert g % 256 == 0 and g >= GUARD_MIN and rear >= g and (g + nbytes + rear) % 256 == 0
    return g, g + nbytes + rear


class GuardedBuffer:
    """One device allocation [guard | tensor | guard].  The host image is built in numpy (`host`), uploaded once; `ptr` is the device
    address of the tensor, `download()` returns (tensor, front guard bytes, rear guard bytes)."""

    def __init__(self, array, guard_bits, guard=GUARD_MIN):
        a = np.ascontiguousarray(array)
        self.shape, self.dtype, self.nbytes = a.shape, a.dtype, a.nbytes
        self.off, self.total = guard_layout(a.nbytes, guard)
        self.host = np.empty(self.total, np.uint8)
        self.fill_guards(guard_bits)
        self.host[self.off:self.off + self.nbytes] = a.reshape(-1).view(np.uint8)
        self.dev = None

    def fill_guards(self, bits):
        """Fill both guards with the 32-bit pattern `bits` (bytes in memory order; the rear guard's phase continues from the tensor's end,
        so a dword-aligned read past the tensor sees whole patterns when the tensor's size is a multiple of 4)."""
        pat = np.array([bits], np.uint32).view(np.uint8)
        self.host[:self.off] = np.tile(pat, self.off // 4)
        rear = self.total - self.off - self.nbytes
        self.host[self.off + self.nbytes:] = np.tile(pat, rear // 4 + 1)[:rear]
        self.guard_bits = bits
        return self

    def set(self, array):
        a = np.ascontiguousarray(array)
        assert a.nbytes == self.nbytes
        self.host[self.off:self.off + self.nbytes] = a.reshape(-1).view(np.uint8)
        return self

    def tensor_host(self):
        return self.host[self.off:self.off + self.nbytes].view(self.dtype).reshape(self.shape)

    def upload(self):
        import torch
        if self.dev is None:
            self.dev = torch.empty(self.total, dtype=torch.uint8, device="cuda")
            assert self.dev.data_ptr() % 256 == 0
        self.dev.copy_(torch.from_numpy(self.host))
        return self

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.off

    def download(self):
        raw = self.dev.cpu().numpy()
        t = raw[self.off:self.off + self.nbytes].view(self.dtype).reshape(self.shape).copy()
        return t, raw[:self.off], raw[self.off + self.nbytes:]

    def read_checked(self, what=""):
        """The tensor, after asserting that both guards still hold exactly what was uploaded (byte-identical)."""
        t, front, rear = self.download()
        assert np.array_equal(front, self.host[:self.off]), f"{what}: front guard overwritten at byte {int(np.argmax(front != self.host[:self.off]))}"
        r0 = self.host[self.off + self.nbytes:]
        assert np.array_equal(rear, r0), f"{what}: rear guard overwritten at byte {int(np.argmax(rear != r0))} past the tensor"
        return t
