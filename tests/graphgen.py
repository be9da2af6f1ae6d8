"""Seeded generator of small ONNX graphs over exactly the vocabulary the planner accepts (facerecognizeonnx_amd/csrc/plan.cpp).

`make_graph(seed, d)` writes `<d>/g<seed>.onnx` with synth/onnx_writer.OnnxBuilder and returns (path, spec); `spec` is a short text form
of the graph that the tests print on failure (the .onnx stays behind in `d` for a replay).  Everything is drawn from
np.random.default_rng(seed).  Seeds below MOTIF_BASE are random compositions of the blocks below; `MOTIFS` are fixed graphs, each aimed
at one planner rule or engine decision, and `REGRESSIONS` are reduced graphs of bugs these tests found.  `REJECTS` lie just outside the
vocabulary: the planner must refuse them cleanly.

Values stay O(1): every convolution's weights are rescaled by the measured standard deviation of its output on a sample input, biases
are O(0.1), and every BatchNormalization takes its statistics from the value it normalises (a fp64 torch forward pass runs alongside the
construction).  An output that grows large is a bug of this module.

Thresholds are not restated here: the shape choices cite the predicate they aim at (file:line at the time of writing).
"""
from __future__ import annotations

import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from facerecognizeonnx_amd.synth.onnx_writer import OnnxBuilder

f32 = np.float32


class Net:
    """A graph under construction: ONNX nodes plus the fp64 value of every tensor on one sample input."""

    def __init__(self, rng, H, W, name="fuzz"):
        self.rng = rng
        self.b = OnnxBuilder(name)
        self.H, self.W = int(H), int(W)
        self.b.add_input("input", [1, 3, self.H, self.W])
        self.v = {"input": torch.from_numpy(rng.uniform(-1, 1, (1, 3, self.H, self.W)))}
        self.spec = [f"input {self.H}x{self.W}"]
        self.outs = []
        self.n = 0

    # ------------------------------------------------------------------ helpers
    def C(self, x):
        return int(self.v[x].shape[1])

    def hw(self, x):
        return int(self.v[x].shape[2]), int(self.v[x].shape[3])

    def _name(self):
        self.n += 1
        return f"t{self.n}"

    def _put(self, op, ins, val, text, **attrs):
        y = self._name()
        self.b.node(op, ins, [y], **attrs)
        self.v[y] = val
        self.spec.append(f"{y}={text}")
        return y

    def _init(self, arr):
        return self.b.init(self.b.uid("w"), np.ascontiguousarray(arr))

    # ------------------------------------------------------------------ vocabulary
    def conv(self, x, cout, k=3, s=1, g=1, bias=True, gain=1.0):
        cin = self.C(x)
        p = 1 if k == 3 else 0
        w = self.rng.standard_normal((cout, cin // g, k, k))
        y = F.conv2d(self.v[x], torch.from_numpy(w), None, s, p, 1, g)
        sd = float(y.std()) if y.numel() > 1 else float(y.abs().max())
        w *= gain / (sd if sd > 0 else 1.0)
        ins = [x, self._init(w.astype(f32))]
        bb = self.rng.normal(0, 0.1, cout) if bias else np.zeros(cout)
        if bias:
            ins.append(self._init(bb.astype(f32)))
        y = F.conv2d(self.v[x], torch.from_numpy(w.astype(f32).astype(np.float64)),
                     torch.from_numpy(bb.astype(f32).astype(np.float64)), s, p, 1, g)
        return self._put("Conv", ins, y, f"conv{k}x{k}/s{s}{'/g%d' % g if g > 1 else ''}({x})->{cout}",
                         kernel_shape=[k, k], strides=[s, s], pads=[p] * 4, group=g)

    def dw(self, x, s=1):
        return self.conv(x, self.C(x), 3, s, g=self.C(x))

    def dwglobal(self, x):
        h, w = self.hw(x)
        assert h == w
        c = self.C(x)
        wt = self.rng.standard_normal((c, 1, h, w)) / h
        bb = self.rng.normal(0, 0.1, c)
        y = F.conv2d(self.v[x], torch.from_numpy(wt.astype(f32).astype(np.float64)), torch.from_numpy(bb.astype(f32).astype(np.float64)),
                     1, 0, 1, c)
        return self._put("Conv", [x, self._init(wt.astype(f32)), self._init(bb.astype(f32))], y, f"dwglobal{h}({x})",
                         kernel_shape=[h, w], strides=[1, 1], pads=[0, 0, 0, 0], group=c)

    def bn(self, x):
        val = self.v[x]
        c = self.C(x)
        if val.dim() == 4:
            mu = val.mean((0, 2, 3)).numpy() + self.rng.normal(0, 0.05, c)
            var = val.var((0, 2, 3), unbiased=False).numpy() * self.rng.uniform(0.8, 1.25, c) + 0.01
        else:
            mu = self.rng.normal(0, 0.1, c)
            var = np.full(c, float((val ** 2).mean())) * self.rng.uniform(0.8, 1.25, c) + 0.01
        g = self.rng.uniform(0.5, 1.5, c)
        be = self.rng.normal(0, 0.1, c)
        ps = [a.astype(f32) for a in (g, be, mu, var)]
        y = F.batch_norm(val, *[torch.from_numpy(a.astype(np.float64)) for a in (ps[2], ps[3], ps[0], ps[1])], False, 0.0, 1e-5)
        return self._put("BatchNormalization", [x] + [self._init(a) for a in ps], y, f"bn({x})", epsilon=1e-5)

    def relu(self, x):
        return self._put("Relu", [x], F.relu(self.v[x]), f"relu({x})")

    def sigmoid(self, x):
        return self._put("Sigmoid", [x], torch.sigmoid(self.v[x]), f"sigmoid({x})")

    def prelu(self, x, per_channel=True):
        c = self.C(x)
        sl = self.rng.uniform(0.05, 0.4, (c, 1, 1) if per_channel else (1,)).astype(f32)
        y = F.prelu(self.v[x], torch.from_numpy(sl.reshape(-1).astype(np.float64)))
        return self._put("PRelu", [x, self._init(sl)], y, f"prelu{'C' if per_channel else '1'}({x})")

    def act(self, x, kind):
        return {"relu": self.relu, "prelu": self.prelu, "prelu1": lambda t: self.prelu(t, False), "sigmoid": self.sigmoid,
                "none": lambda t: t}[kind](x)

    def add(self, a, b):
        return self._put("Add", [a, b], self.v[a] + self.v[b], f"add({a},{b})")

    def up2(self, x, op="Resize"):
        y = F.interpolate(self.v[x], scale_factor=2, mode="nearest")
        if op == "Upsample":
            return self._put("Upsample", [x, self._init(np.array([1, 1, 2, 2], f32))], y, f"upsample2({x})", mode="nearest")
        return self._put("Resize", [x, self._init(np.zeros(0, f32)), self._init(np.array([1, 1, 2, 2], f32))], y, f"resize2({x})",
                         mode="nearest", coordinate_transformation_mode="asymmetric", nearest_mode="floor")

    def const_op(self, x, op, per_channel=True):
        c = self.C(x)
        shp = (1, c, 1, 1) if per_channel and self.v[x].dim() == 4 else (1, c) if per_channel else ()
        if op in ("Mul", "Div"):
            k = (self.rng.uniform(0.5, 2.0, shp) * self.rng.choice([-1, 1], shp)).astype(f32)
        else:
            k = self.rng.normal(0, 0.3, shp).astype(f32)
        t = torch.from_numpy(np.asarray(k, np.float64))
        y = {"Mul": torch.mul, "Div": torch.div, "Add": torch.add, "Sub": torch.sub}[op](self.v[x], t)
        return self._put(op, [x, self._init(np.asarray(k))], y, f"{op.lower()}{'C' if per_channel else '1'}({x})")

    def passthrough(self, x, op="Identity"):
        return self._put(op, [x], self.v[x], f"{op.lower()}({x})")

    # ------------------------------------------------------------------ outputs
    def head_nhwc(self, x):
        t = self._put("Transpose", [x], self.v[x].permute(0, 2, 3, 1), f"nhwc({x})", perm=[0, 2, 3, 1])
        c = self.C(x)
        y = self._put("Reshape", [t, self._init(np.array([-1, c], np.int64))], self.v[t].reshape(-1, c), f"rows({t})")
        self._output(y)
        return y

    def head_fc(self, x, n_out, matmul=False, nhwc=False, bn=False):
        if nhwc:
            x = self._put("Transpose", [x], self.v[x].permute(0, 2, 3, 1), f"nhwc({x})", perm=[0, 2, 3, 1])
        f = self._put("Flatten", [x], self.v[x].flatten(1), f"flat({x})", axis=1)
        K = int(self.v[f].shape[1])
        w = self.rng.standard_normal((n_out, K)) / np.sqrt(K)
        y = self.v[f] @ torch.from_numpy(w.T)
        w /= max(float(y.std()), 1e-6) if n_out > 1 else 1.0
        w = w.astype(f32)
        if matmul:
            y = self._put("MatMul", [f, self._init(np.ascontiguousarray(w.T))], self.v[f] @ torch.from_numpy(w.T.astype(np.float64)),
                          f"matmul({f})->{n_out}")
        else:
            bb = self.rng.normal(0, 0.1, n_out).astype(f32)
            y = self._put("Gemm", [f, self._init(w), self._init(bb)],
                          self.v[f] @ torch.from_numpy(w.T.astype(np.float64)) + torch.from_numpy(bb.astype(np.float64)),
                          f"gemm({f})->{n_out}", transB=1)
        if bn:
            y = self.bn(y)
        self._output(y)
        return y

    def head_flat(self, x):
        """A flattened 1x1 value straight out (NCHW order is storage order at H = W = 1), with a standalone BN on the flat value."""
        assert self.hw(x) == (1, 1)
        f = self._put("Flatten", [x], self.v[x].flatten(1), f"flat({x})", axis=1)
        y = self.bn(f)
        self._output(y)
        return y

    def _out_raw(self, y, c):
        """Channels-last output of a value the generator does not evaluate (the reject graphs)."""
        t = self.b.node("Transpose", [y], ["yt"], perm=[0, 2, 3, 1])
        r = self.b.node("Reshape", [t, self._init(np.array([-1, c], np.int64))], ["rows"])
        self.b.add_output(r, [-1, c])

    def _output(self, y):
        self.b.add_output(y, list(self.v[y].shape))
        self.outs.append(y)
        self.spec.append(f"out {y}")

    def save(self, path):
        for o in self.outs:
            m = float(self.v[o].abs().max())
            assert 1e-3 < m < 1e3, f"graphgen: output {o} has scale {m} (generator bug)\n" + "\n".join(self.spec)
        self.b.save(path)
        return path, "\n".join(self.spec)


# ---------------------------------------------------------------------------------------------------- blocks
def conv_act(n, x, cout, k=3, s=1, act=None, bn=None):
    """Conv (+ folded BN) (+ folded activation)."""
    r = n.rng
    y = n.conv(x, cout, k, s)
    if bn if bn is not None else r.random() < 0.4:
        y = n.bn(y)                                                   # plan.cpp step 2: folded into the weights
    return n.act(y, act or r.choice(["relu", "prelu", "prelu1", "sigmoid", "none"]))


def res_block(n, x, shortcut_first=None):
    """y = conv3(act(conv3(x))) + x: the Add folds into the second conv (+res)."""
    r = n.rng
    c = n.C(x)
    first = r.random() < 0.5 if shortcut_first is None else shortcut_first
    y = conv_act(n, x, c, 3, 1, act=r.choice(["relu", "prelu"]))
    y = n.conv(y, c, 3, 1)
    return n.add(x, y) if first else n.add(y, x)


def proj_block(n, x, cout, s, shortcut_first):
    """IResNet block with a projection: bn1(x) -> conv3 s1 -> prelu -> conv3 s -> (+ 1x1 s shortcut of x).
    bn1 becomes x's producer's second output (+bn2nd), conv1 reads it (bn<-op when conv1 is the only reader), the Add folds into conv2
    (+res) and the shortcut can run in conv2's K loop (sc<-op: plan.cpp:813-831, Cin % 32 == 0)."""
    sc = n.conv(x, cout, 1, s) if shortcut_first else None
    y = n.bn(x)
    y = n.conv(y, cout, 3, 1)
    y = n.bn(y)
    y = n.prelu(y)
    y = n.conv(y, cout, 3, s)
    y = n.bn(y)
    if sc is None:
        sc = n.conv(x, cout, 1, s)
    return n.add(y, sc)


def ires_block(n, x):
    """Identity IResNet block: bn1(x) -> conv3 -> prelu -> conv3 -> + x."""
    c = n.C(x)
    y = n.bn(x)
    y = n.conv(y, c, 3, 1)
    y = n.prelu(y)
    y = n.conv(y, c, 3, 1)
    return n.add(y, x)


def dwpw_block(n, x, s=1, cout=None, acts=("relu", "relu")):
    y = n.dw(x, s)
    y = n.act(y, acts[0])
    y = n.conv(y, cout or n.C(x), 1, 1)
    return n.act(y, acts[1])


def gconv_block(n, x, g):
    y = n.conv(x, n.C(x), 3, 1, g=g)
    return n.act(y, n.rng.choice(["relu", "prelu", "none"]))


def siblings(n, x, couts, k=3):
    """2-3 sibling convs on one input with <= 32 channels in all: plan.cpp 7b merges them ([merged xN])."""
    return [n.act(n.conv(x, c, k, 1), n.rng.choice(["relu", "sigmoid", "none"])) for c in couts]


def up2_res(n, x, cout):
    """FPN-style: conv3 s1 (x) + Resize x2 (conv s2 (x)) -> +res(up2x).  Needs even sides."""
    lo = n.conv(x, cout, 3, 2)
    hi = n.conv(x, cout, 1, 1)
    return n.add(hi, n.up2(lo))


def standalone(n, x):
    """Ops that stay ops (their input is no single-use conv output): AFFINE, ACT, ADD, UPSAMPLE."""
    r = n.rng
    a = n.relu(x)                                                      # x has another reader below: an ACT op
    b = n.const_op(x, r.choice(["Mul", "Add", "Sub", "Div"]), per_channel=bool(r.random() < 0.6))
    y = n.add(a, b)                                                    # neither side is a conv: an ADD op
    y = n.act(y, r.choice(["sigmoid", "prelu", "prelu1"]))
    return y


# ---------------------------------------------------------------------------------------------------- random graphs
def _random(seed):
    r = np.random.default_rng(seed)
    H, W = (int(v) for v in r.integers(17, 97, 2))
    n = Net(r, H, W, f"g{seed}")
    c = int(r.choice([8, 16, 32]))
    x = conv_act(n, "input", c, 3, int(r.choice([1, 2])))
    nout = int(r.integers(1, 5))
    for _ in range(int(r.integers(3, 8))):
        h, w = n.hw(x)
        c = n.C(x)
        kinds = ["conv", "res", "dwpw", "gconv", "standalone", "siblings", "bnconv", "pass", "act_bn"]
        if h * w <= 1600:
            kinds.append("upsample")
        if h % 2 == 0 and w % 2 == 0 and h >= 4 and w >= 4:
            kinds.append("up2")
        if min(h, w) >= 6:
            kinds += ["down", "proj"]
        k = r.choice(kinds)
        if k == "conv":
            x = conv_act(n, x, int(r.choice([8, 16, 24, 32, 64])), int(r.choice([1, 3])), 1)
        elif k == "down":
            x = conv_act(n, x, int(r.choice([16, 32, 64])), int(r.choice([1, 3])), 2)
        elif k == "res":
            x = res_block(n, x)
        elif k == "dwpw":
            x = dwpw_block(n, x, int(r.choice([1, 2])) if min(h, w) >= 6 else 1, int(r.choice([c, 2 * c])) if c <= 32 else c)
        elif k == "gconv":
            g = int(r.choice([c // 2, c // 4, 2])) if c >= 8 else 2
            x = gconv_block(n, x, max(g, 1))
        elif k == "standalone":
            x = standalone(n, x)
        elif k == "siblings":
            parts = siblings(n, x, [[8, 8], [16, 16], [8, 8, 16], [4, 8, 12]][int(r.integers(4))])
            for p in parts[1:]:
                if len(n.outs) < nout - 1:
                    n.head_nhwc(p)
            x = parts[0]
        elif k == "bnconv":
            x = ires_block(n, x)
        elif k == "proj":
            x = proj_block(n, x, int(r.choice([32, 64])), int(r.choice([1, 2])), bool(r.random() < 0.5))
        elif k == "up2":
            x = n.relu(up2_res(n, x, c))
        elif k == "act_bn":
            x = n.bn(conv_act(n, x, c, 3, 1, act=str(r.choice(["relu", "prelu", "sigmoid"])), bn=False))   # bn2nd-only
        elif k == "upsample":
            x = conv_act(n, n.up2(x, str(r.choice(["Resize", "Upsample"]))), c, 3, 1)
        else:
            x = n.passthrough(x, str(r.choice(["Identity", "Dropout"])))
        if len(n.outs) < nout - 1 and r.random() < 0.3:
            n.head_nhwc(x)
    if r.random() < 0.5:
        n.head_nhwc(x)
    else:
        if n.hw(x)[0] * n.hw(x)[1] * n.C(x) > 8192:
            x = conv_act(n, x, 16, 3, 2)
        n.head_fc(x, int(r.choice([8, 16, 32])), matmul=bool(r.random() < 0.4), nhwc=bool(r.random() < 0.3), bn=bool(r.random() < 0.3))
    return n


# ---------------------------------------------------------------------------------------------------- named motifs
def _m_shared_output(n):
    """A tensor read by three ops and exported itself."""
    x = conv_act(n, "input", 16, 3, 1, act="relu", bn=False)
    a = n.conv(x, 16, 3, 1)
    b = n.conv(x, 8, 1, 1)
    c = n.relu(x)
    n.head_nhwc(x)
    n.head_nhwc(n.add(a, c))
    n.head_nhwc(b)


def _m_proj_strided(n, first):
    """Strided projection blocks, shortcut written before / after conv1 (sc<-op, bn<-op, +bn2nd)."""
    x = conv_act(n, "input", 32, 3, 1, act="prelu", bn=True)
    x = proj_block(n, x, 32, 2, first)
    x = proj_block(n, x, 64, 2, not first)
    x = ires_block(n, x)
    n.head_fc(x, 32, bn=True)


def _m_proj_s1_wino(n, first):
    """Stride-1 projection block with >= 128 channels: the consumer may run as Winograd F(4x4) at large batches, so its shortcut must
    NOT be folded into the K loop there (engine.cpp:235; the 5af4c7f bug)."""
    x = conv_act(n, "input", 32, 3, 2, act="relu", bn=True)
    x = proj_block(n, x, 128, 1, first)
    x = proj_block(n, x, 128, 1, not first)
    n.head_nhwc(x)


def _m_bn_link(n):
    """bn<-op on Winograd-eligible convs (>= 128 channels, kWinoMinCin engine.cpp:87) with the shortcut written first, so the plain
    output's last listed reader comes before conv1 (plan.cpp:795-811) and the producer's second output is skipped at batches where the
    consumer runs as Winograd (engine.cpp:451-454)."""
    x = conv_act(n, "input", 128, 3, 2, act="prelu", bn=True)
    x = proj_block(n, x, 128, 1, True)
    x = ires_block(n, x)
    n.head_nhwc(x)


def _m_merge(n):
    """2 and 3 sibling convs (<= 32 channels in all: plan.cpp:701) on a 64-channel input (wino2's merged epilogue, conv_wino2.hip:389)."""
    x = conv_act(n, "input", 64, 3, 2, act="relu", bn=False)
    for p in siblings(n, x, [8, 8, 16]) + siblings(n, x, [16, 16], k=1):
        n.head_nhwc(p)


def _m_dwpw(n, s):
    """DW->PW pairs just above and just below the fusion threshold (plan.cpp:743)."""
    x = conv_act(n, "input", 16, 3, 1, act="relu", bn=False)
    x = dwpw_block(n, x, s, 32)
    y = dwpw_block(n, x, 2, 32)                                         # the next pair is well below the threshold
    n.head_nhwc(y)


def _m_dw_forms(n, c):
    """Depthwise 3x3 convs in all four forms of launch_dwconv3x3 (ops_misc.hip:248-268): the lean kernel (C >= 8, activation none /
    ReLU / PReLU) and the generic ones (C < 8 or a sigmoid: dwconv3x3_kernel at stride 1, dwconv3x3_hstrip_kernel at stride 2), each at
    stride 1 and 2.  Maps stay below the DW->PW threshold and no depthwise output feeds a 1x1 conv alone, so none of them is fused."""
    x = conv_act(n, "input", c, 3, 1, act="relu", bn=False)
    a = n.act(n.dw(x, 1), "relu")                                      # c = 4: generic s1; c >= 8: lean s1
    b = n.act(n.dw(a, 2), "prelu")                                     # c = 4: generic s2 (hstrip); c >= 8: lean s2
    n.head_nhwc(b)
    y = n.sigmoid(n.dw(x, 2))                                          # sigmoid: generic s2 at any C
    y = n.sigmoid(n.dw(y, 1))                                          # ... and generic s1
    n.head_nhwc(n.add(y, n.relu(b)))


def _m_front(n, stem_stride):
    """16-channel stem + DW->PW (front_fused_ok, dwpw_mfma.hip:774)."""
    x = conv_act(n, "input", 16, 3, stem_stride, act="relu", bn=True)
    x = dwpw_block(n, x, 1, 32)
    n.head_nhwc(x)
    n.head_nhwc(conv_act(n, x, 16, 3, 2, act="sigmoid"))


def _m_halo(n):
    """16-channel 3x3 s1 convs on maps >= 16x16 (conv_halo_ok, conv_halo.hip:251; Ho*Wo >= 400 at engine.cpp:176)."""
    x = conv_act(n, "input", 16, 3, 1, act="relu", bn=False)
    a = conv_act(n, x, 32, 3, 1, act="relu", bn=False)
    b = res_block(n, conv_act(n, x, 16, 3, 1, act="none", bn=False), False)
    n.head_nhwc(a)
    n.head_nhwc(b)


def _m_wino2(n):
    """64-channel 3x3 s1 convs (wino2_ok in conv_wino2.hip)."""
    x = conv_act(n, "input", 64, 3, 2, act="relu", bn=False)
    x = conv_act(n, x, 64, 3, 1, act="relu", bn=False)
    x = res_block(n, x, False)
    n.head_nhwc(x)


def _m_wino_chain(n):
    """Chains of 3x3 s1 convs with >= 128 channels on a 14x14 map (side 4k+2: the mixed F(4x4)/F(2x2) tiling, wino_mix_layout in
    winograd.hip) and on a 7x7 map, with fused transforms between consecutive layers (engine.cpp:260-279, 515-527)."""
    x = conv_act(n, "input", 32, 3, 2, act="relu", bn=True)
    x = conv_act(n, x, 128, 3, 1, act="relu", bn=True)
    x = conv_act(n, x, 128, 3, 1, act="prelu", bn=True)
    x = ires_block(n, x)
    n.head_nhwc(x)
    y = conv_act(n, x, 128, 3, 2, act="relu", bn=True)
    y = conv_act(n, y, 128, 3, 1, act="relu", bn=True)
    y = conv_act(n, y, 128, 3, 1, act="none", bn=True)
    n.head_fc(y, 16)


def _m_fc_splitk(n):
    """Flatten + Gemm with K >= 8192 at B = 1: split-K cuts each tile into many slabs (conv_fixup_kernel)."""
    x = conv_act(n, "input", 32, 3, 2, act="relu", bn=False)
    n.head_fc(x, 64)                                                   # K = 32 * 24 * 24 = 18432 (NCHW flatten: permuted K)
    n.head_fc(n.conv(x, 16, 1, 1), 32, matmul=True, nhwc=True)


def _m_pw_tall(n):
    """1x1 s1 and 3x3 s1 layers with enough pixels at B_hi for conv_pw_kernel / conv_tall_kernel (conv_plan.h: launch_pw's
    eligibility predicate conv_pw_bn, conv_tall_kernel's take-over predicate conv_tall_plan)."""
    x = conv_act(n, "input", 32, 3, 1, act="relu", bn=False)
    a = conv_act(n, x, 32, 1, 1, act="relu", bn=False)
    b = conv_act(n, a, 32, 3, 1, act="prelu", bn=False)
    n.head_nhwc(b)


def _m_grouped(n):
    """Grouped convs: G = 2 / 4 channels per group (GCONV), other G (block-diagonal CONV, plan.cpp:543-551), global depthwise
    (DWGLOBAL) and a standalone BN on the flattened 1x1 value."""
    x = conv_act(n, "input", 16, 3, 2, act="relu", bn=False)
    x = gconv_block(n, x, 8)
    x = gconv_block(n, x, 4)
    x = n.conv(x, 16, 3, 1, g=2)
    x = n.conv(x, 16, 1, 1, g=4)
    x = conv_act(n, x, 32, 3, 2, act="prelu", bn=True)
    n.head_nhwc(x)
    n.head_flat(n.dwglobal(x))


def _m_up2(n):
    """+res(up2x), a standalone x2 upsample (Resize and Upsample), standalone ACT / ADD / AFFINE."""
    x = conv_act(n, "input", 16, 3, 2, act="relu", bn=False)
    y = n.relu(up2_res(n, x, 16))
    u = n.up2(n.conv(x, 16, 3, 2), "Upsample")
    y = n.add(n.relu(u), y)
    n.head_nhwc(standalone(n, y))
    n.head_nhwc(n.passthrough(x, "Dropout"))


def _m_act_bn(n):
    """Conv -> activation -> BN: the BN cannot fold and becomes the conv's only written output (bn2nd-only)."""
    x = n.bn(conv_act(n, "input", 16, 3, 1, act="relu", bn=False))
    y = n.bn(conv_act(n, x, 32, 3, 2, act="prelu", bn=True))
    n.head_nhwc(y)
    n.head_fc(n.bn(conv_act(n, y, 16, 1, 1, act="sigmoid", bn=False)), 8)


MOTIF_BASE = 1000
MOTIFS = {                                                             # seed -> (input H, W, builder)
    1000: ("shared_output", (33, 41), _m_shared_output),
    1001: ("proj_strided_sc_first", (48, 48), lambda n: _m_proj_strided(n, True)),
    1002: ("proj_strided_sc_after", (40, 56), lambda n: _m_proj_strided(n, False)),
    1003: ("proj_s1_wino", (28, 28), lambda n: _m_proj_s1_wino(n, True)),
    1004: ("proj_s1_wino_after", (24, 32), lambda n: _m_proj_s1_wino(n, False)),
    1005: ("bn_link", (28, 28), _m_bn_link),
    1006: ("merge", (40, 34), _m_merge),
    1007: ("dwpw_s1_above", (40, 40), lambda n: _m_dwpw(n, 1)),
    1008: ("dwpw_s1_below", (39, 41), lambda n: _m_dwpw(n, 1)),
    1009: ("dwpw_s2_above", (160, 160), lambda n: _m_dwpw(n, 2)),
    1010: ("dwpw_s2_below", (158, 160), lambda n: _m_dwpw(n, 2)),
    1011: ("front_s1", (48, 50), lambda n: _m_front(n, 1)),
    1012: ("front_s2", (96, 90), lambda n: _m_front(n, 2)),
    1013: ("halo", (24, 30), _m_halo),
    1014: ("wino2", (36, 44), _m_wino2),
    1015: ("wino_chain", (28, 28), _m_wino_chain),
    1016: ("wino_chain_odd", (26, 27), _m_wino_chain),
    1017: ("fc_splitk", (48, 48), _m_fc_splitk),
    1018: ("pw_tall", (32, 32), _m_pw_tall),
    1019: ("grouped", (30, 30), _m_grouped),
    1020: ("up2", (36, 44), _m_up2),
    1021: ("dwpw_s2_above_odd", (163, 171), lambda n: _m_dwpw(n, 2)),
    1022: ("grouped_odd", (34, 34), _m_grouped),
    1023: ("act_bn", (29, 31), _m_act_bn),
    1024: ("dw_forms_c4", (27, 34), lambda n: _m_dw_forms(n, 4)),
    1025: ("dw_forms_c16", (30, 23), lambda n: _m_dw_forms(n, 16)),
}

RANDOM_SEEDS = list(range(32))
REGRESSIONS = {}                                                       # seed -> (name, (H, W), builder): reduced graphs of bugs found
ALL_SEEDS = RANDOM_SEEDS + sorted(MOTIFS) + sorted(REGRESSIONS)


def make_graph(seed, d):
    """-> (onnx_path, spec) of graph `seed`, written to directory `d`."""
    seed = int(seed)
    named = MOTIFS.get(seed) or REGRESSIONS.get(seed)
    if named:
        name, (H, W), fn = named
        n = Net(np.random.default_rng(seed), H, W, name)
        n.spec[0] += f"  [{name}]"
        fn(n)
    else:
        n = _random(seed)
    return n.save(os.path.join(d, f"g{seed}.onnx"))


# ---------------------------------------------------------------------------------------------------- reading a plan
_OP_RE = re.compile(r"^(\d+) (\S+) k(\d+)s(\d+) (\d+)x(\d+)x(\d+) -> (\d+)x(\d+)x(\d+)(.*)$")
_TENSORS_RE = re.compile(r"\[in t(-?\d+) out t(-?\d+) out2 t(-?\d+) in2 t(-?\d+) res t(-?\d+)(?: outs ([t\d,]+))?\]")


def parse_ops(desc):
    """Plan::describe() -> one dict per op: i, kind ("DW+PW s1" / "DW+PW s2" for the fused pairs), ks, stride, H, W, Cin, Ho, Wo, Cout,
    the line itself (text), the tensors it reads and writes, its plain output (out) and its bn<-op / sc<-op links (-1: none)."""
    ops = []
    for line in desc.splitlines():
        m = _OP_RE.match(line)
        if not m:
            continue
        i, kind = int(m.group(1)), m.group(2)
        if kind == "DW+PW":
            kind = "DW+PW s2" if "(depthwise s2)" in line else "DW+PW s1"
        br = _TENSORS_RE.search(line)
        assert br, line
        tin, tout, tout2, tin2, tres = (int(br.group(k)) for k in range(1, 6))
        outs = [int(t[1:]) for t in br.group(6).split(",")] if br.group(6) else []
        bn = re.search(r"bn<-op(\d+)", line)
        sc = re.search(r"sc<-op(\d+)", line)
        ops.append(dict(i=i, kind=kind, ks=int(m.group(3)), stride=int(m.group(4)), H=int(m.group(5)), W=int(m.group(6)),
                        Cin=int(m.group(7)), Ho=int(m.group(8)), Wo=int(m.group(9)), Cout=int(m.group(10)), text=line,
                        reads=[t for t in (tin, tin2, tres) if t >= 0], writes=[t for t in [tout, tout2] + outs if t >= 0],
                        out=tout, bn=int(bn.group(1)) if bn else -1, sc=int(sc.group(1)) if sc else -1))
    return ops


def dw_form(op):
    """Which kernel launch_dwconv3x3 (ops_misc.hip:254-256) runs for a DWCONV op of these small maps: "lean" from 8 channels on with no
    activation, ReLU or PReLU, "generic" otherwise — e.g. "generic s2" is dwconv3x3_hstrip_kernel."""
    lean = op["Cin"] >= 8 and "+sigmoid" not in op["text"]
    return f"{'lean' if lean else 'generic'} s{op['stride']}"


# ---------------------------------------------------------------------------------------------------- outside the vocabulary
def _rej_conv_attr(n, **attrs):
    c = 8
    w = n._init((n.rng.standard_normal((c, 3, 3, 3)) * 0.2).astype(f32))
    y = n.b.node("Conv", ["input", w], ["y"], kernel_shape=[3, 3], **attrs)
    n.v["y"] = None
    n._out_raw(y, c)


def _rej_dilation(n):
    _rej_conv_attr(n, strides=[1, 1], pads=[2, 2, 2, 2], dilations=[2, 2])


def _rej_auto_pad(n):
    _rej_conv_attr(n, strides=[1, 1], auto_pad="SAME_UPPER")


def _rej_resize3(n):
    x = n.conv("input", 8, 3, 1)
    y = n.b.node("Resize", [x, n._init(np.zeros(0, f32)), n._init(np.array([1, 1, 3, 3], f32))], ["y"], mode="nearest")
    n._out_raw(y, 8)


def _rej_resize_linear(n):
    x = n.conv("input", 8, 3, 1)
    y = n.b.node("Resize", [x, n._init(np.zeros(0, f32)), n._init(np.array([1, 1, 2, 2], f32))], ["y"], mode="linear")
    n._out_raw(y, 8)


def _rej_broadcast_add(n):
    """Both operands are standalone activations (their inputs have other readers), so the Add stays an ADD op instead of a conv's
    fused residual, and reaches the planner's own shape check."""
    x = n.conv("input", 8, 3, 1)
    p = n.conv(x, 8, 3, 2)
    n.head_nhwc(p)
    y = n.b.node("Add", [n.relu(x), n.relu(p)], ["y"])
    n._out_raw(y, 8)


def _rej_grouped_c6(n):
    x = n.conv("input", 6, 3, 1)
    y = n.b.node("Conv", [x, n._init((n.rng.standard_normal((6, 2, 3, 3)) * 0.3).astype(f32))], ["y"], kernel_shape=[3, 3],
                 pads=[1, 1, 1, 1], group=3)
    n._out_raw(y, 6)


def _rej_reshape_nchw(n):
    x = n.conv("input", 8, 3, 2)
    y = n.b.node("Reshape", [x, n._init(np.array([-1, 8], np.int64))], ["y"])         # NCHW order: would need a transpose
    n.b.add_output(y, [-1, 8])


def _rej_conv5_w(n):
    c = 8
    w = n._init((n.rng.standard_normal((c, 3, 5, 5)) * 0.2).astype(f32))
    y = n.b.node("Conv", ["input", w], ["y"], kernel_shape=[5, 5], pads=[2, 2, 2, 2])
    n._out_raw(y, c)


def _rej_nchw_output(n):
    x = n.conv("input", 8, 3, 1)
    n.b.add_output(x, [1, 8, n.H, n.W])


def _rej_maxpool(n):
    x = n.conv("input", 8, 3, 1)
    y = n.b.node("MaxPool", [x], ["y"], kernel_shape=[2, 2], strides=[2, 2])
    n._out_raw(y, 8)


def _rej_sub_const_first(n):
    x = n.conv("input", 8, 3, 1)
    y = n.b.node("Sub", [n._init(np.ones((1, 8, 1, 1), f32)), n.relu(x)], ["y"])
    n._out_raw(y, 8)


REJECTS = {
    "dilation": _rej_dilation,
    "auto_pad": _rej_auto_pad,
    "resize_x3": _rej_resize3,
    "resize_linear": _rej_resize_linear,
    "broadcast_add": _rej_broadcast_add,
    "grouped_c6": _rej_grouped_c6,
    "reshape_nchw": _rej_reshape_nchw,
    "conv5x5": _rej_conv5_w,
    "nchw_output": _rej_nchw_output,
    "maxpool": _rej_maxpool,
    "const_minus_tensor": _rej_sub_const_first,
}


def make_reject(name, d):
    n = Net(np.random.default_rng(7), 20, 24, "rej_" + name)
    REJECTS[name](n)
    path = os.path.join(d, f"rej_{name}.onnx")
    n.b.save(path)
    return path
