"""Seeded random ONNX graphs (tests/graphgen.py) through the planner AND the engine on the GPU, against torch fp64 and the oracle.

Each graph runs in a detector handle (fh_det_run_network_dev on u8 frames of the graph's own size, every output read back) and, when it
has a single output, in a recogniser handle too (fh_rec_embed_aligned_dev, raw output), where the Winograd-fusion and shortcut-fold
switches live.  Batches: B_hi, 1, B_hi again on new frames (stale arena contents present; a repeated call must be bitwise identical),
then 3.  B_hi is derived per graph from the engine's batch-dependent predicates so that some eligible layers cross their threshold and
others do not.  Every slot of B = 1 / 3 and the first / middle / last slots of B_hi are held to 1e-4 of the output's scale (2e-4 when a
Winograd F(4x4) layer ran: docs/tolerances.md) against torch fp64 and the oracle, both on the preprocessed input; so is every switch of
the matrix below, and the fused / unfused pairs agree with the default within 1e-5 of scale.  The kernel ledger (fh_timing_collect_ops)
proves that the corpus reaches every timing tag and each small kernel that no other test launches.

FACEHIP_GRAPH_FUZZ_SEEDS=N widens the random part of the corpus to seeds 0 .. N-1.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import api
from oracle import onnx_min, oracle
from oracle import torch_graph as torch_ref
from tests import graphgen as gg
from tests import util

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_RANDOM = int(os.environ.get("FACEHIP_GRAPH_FUZZ_SEEDS", len(gg.RANDOM_SEEDS)))
SEEDS = list(range(N_RANDOM)) + sorted(gg.MOTIFS) + sorted(gg.REGRESSIONS)

K_WINO_MIN_TILES = 256       # engine.cpp:88 kWinoMinTiles (4x4-output tiles per launch)
WINO_MIN_CIN = 128           # engine.cpp:87 kWinoMinCin
WINO2_MIN_BLOCKS = 64        # engine.cpp:94 wino2_min_blocks() default
MIX_MIN_B = 64               # winograd.hip wino_mix_layout: B >= 64
N_CUS = 256                  # conv_mfma.hip num_cus() on an MI355X (the pw / tall predicates count tiles per CU)
TAGS = 13                    # kernels.h KernelTimer::kTags
SMALL_KERNELS = ("ACT", "ADD", "AFFINE", "UPSAMPLE", "DWGLOBAL", "GCONV",
                 "DWCONV lean s1", "DWCONV lean s2", "DWCONV generic s1", "DWCONV generic s2")
BATCH_FORMS = (7, 10, 11, 12)  # Winograd GEMM, conv_tall_kernel, conv_pw_kernel, wino2_kernel: one launch per layer in that form


def _layer_forms(o, sc_targets):
    """The batch-dependent forms op `o` can take, as predicates of the batch: [(name, on(B))].  A layer in one of them launches one
    kernel of BATCH_FORMS."""
    if o["kind"] != "CONV":
        return []
    out = []
    merged = "[merged" in o["text"]
    s1 = o["ks"] == 3 and o["stride"] == 1
    hw = o["Ho"] * o["Wo"]
    if s1 and o["Cin"] >= WINO_MIN_CIN and o["Cin"] % 32 == 0 and o["Cout"] % 4 == 0 and not merged and "+res(up2x)" not in o["text"]:
        tiles = ((o["H"] + 3) // 4) * ((o["W"] + 3) // 4)
        out.append(("wino", lambda B: B * tiles >= K_WINO_MIN_TILES))                          # engine.cpp:493
    elif (s1 and o["Cin"] == 64 and (o["Cout"] % 64 == 0 or (merged and o["Cout"] <= 32)) and "sc<-op" not in o["text"] and
          "+sigmoid" not in o["text"] and "+res(up2x)" not in o["text"]):
        per = (((o["H"] + 1) // 2 + 3) // 4) * (((o["W"] + 1) // 2 + 3) // 4) * ((o["Cout"] + 63) // 64)
        out.append(("wino2", lambda B: B * per // 4 >= WINO2_MIN_BLOCKS))                      # engine.cpp:488, conv_wino2.hip:384-411
    elif (o["ks"] == 1 and o["stride"] == 1 and o["Cout"] <= 32 and o["Cin"] % 4 == 0 and o["Cout"] % 4 == 0 and not merged and
          o["i"] not in sc_targets):
        out.append(("pw", lambda B: B * hw % 128 == 0 and B * hw // 128 >= N_CUS))             # conv_plan.h conv_pw_bn, launch_pw's eligibility (32-wide tiles)
    elif (s1 and o["Cin"] % 32 == 0 and o["Cout"] <= 32 and o["W"] <= 112 and "sc<-op" not in o["text"] and
          "+res(up2x)" not in o["text"]):
        out.append(("tall", lambda B: -(-B * hw // 128) >= N_CUS * 3))                         # conv_plan.h conv_tall_plan, conv_tall_kernel's take-over (128x32 tiles)
    return out


def _forms(ops):
    sc_targets = {o["sc"] for o in ops if o["sc"] >= 0}
    return [f for o in ops for f in _layer_forms(o, sc_targets)]


def _crossings(ops):
    """Per layer form that is off at B = 1: the smallest batch up to 128 at which it is on."""
    return sorted({next(B for B in range(2, 129) if on(B)) for _, on in _forms(ops) if not on(1) and any(on(B) for B in range(2, 129))})


def _on(ops, batch):
    return sum(1 for _, on in _forms(ops) if on(batch))


def b_hi(ops):
    c = _crossings(ops)
    return max(4, c[len(c) // 2]) if c else 5


def _u8(n, h, w, seed):
    return util.frames_u8(n, h, w, seed=seed)


class Refs:
    """fp64 torch and oracle outputs per frame, computed once per graph."""

    def __init__(self, path, det):
        self.tg = torch_ref.TorchGraph(path)
        self.g = onnx_min.load(path)
        self.names = [n for n, _ in self.g.outputs]
        self.det = det
        self.cache = {}

    def get(self, frames, key, idx):
        missing = [i for i in idx if (key, i) not in self.cache]
        if missing:
            pre = self.det_pre if self.det else oracle.rec_preprocess
            x = np.stack([pre(frames[i]) for i in missing])
            t = self.tg.run({self.g.inputs[0][0]: x})
            o = oracle.run_graph(self.g, {self.g.inputs[0][0]: x})
            for j, i in enumerate(missing):
                self.cache[(key, i)] = ([np.asarray(t[nm]).reshape(len(missing), -1)[j] for nm in self.names],
                                        [np.asarray(o[nm]).reshape(len(missing), -1)[j] for nm in self.names])
        return [self.cache[(key, i)] for i in idx]

    @staticmethod
    def det_pre(frame):
        x, scale = oracle.det_preprocess(frame, frame.shape[1], frame.shape[0])
        assert scale == 1.0
        return x


def _collect_tags():
    cap = 1 << 14
    ms, fl, tg = np.zeros(cap), np.zeros(cap), np.zeros(cap, np.int32)
    n = fa.lib().fh_timing_collect_ops(ms.ctypes.data, fl.ctypes.data, tg.ctypes.data, cap)
    assert 0 <= n < cap, fa._lib.last_error()
    return [int(t) for t in tg[:n]]


def _check(got, refs, idx, wino, what, spec):
    """got: per output, one row per entry of idx; refs: Refs.get(...) for the images idx."""
    bar = 2e-4 if wino else 1e-4
    for k, (tref, oref) in enumerate(refs):
        for oi in range(len(tref)):
            g = got[oi][k].reshape(-1)
            scale = max(float(np.abs(tref[oi]).max()), 1e-6)
            for name, r in (("torch fp64", tref[oi]), ("oracle", oref[oi])):
                err = float(np.abs(g - r).max())
                assert np.isfinite(err) and err <= bar * scale, \
                    f"{what}: slot {idx[k]} output {oi} vs {name}: {err:.3g} > {bar} x {scale:.3g}\n{spec}"


def _det_outputs(det, n):
    outs = []
    for i in range(fa.lib().fh_det_num_outputs(det.handle)):
        r, c = C.c_int(), C.c_int()
        p = fa.lib().fh_det_output_dev(det.handle, i, C.byref(r), C.byref(c))
        o = np.empty((n, r.value * c.value), np.float32)
        assert p and fa.lib().fh_memcpy_d2h(o.ctypes.data, p, o.nbytes) == 0, fa._lib.last_error()
        outs.append(o)
    return outs


class DetRunner:
    def __init__(self, path, h, w):
        self.det = fa.FaceDetector()
        assert self.det.loadModel(path), fa._lib.last_error()
        assert self.det.input_size() == (w, h)
        self.h, self.w = h, w

    def run(self, frames):
        n = len(frames)
        d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        fa.lib().fh_timing_enable(1)
        try:
            assert fa.lib().fh_det_run_network_dev(self.det.handle, d.data_ptr(), n, self.h, self.w, self.w * 3,
                                                   self.h * self.w * 3, 0) == n, fa._lib.last_error()
            torch.cuda.synchronize()
            tags = _collect_tags()
        finally:
            fa.lib().fh_timing_enable(0)
        return _det_outputs(self.det, n), tags


class RecRunner:
    def __init__(self, path, h, w):
        self.rec = fa.FaceRecognizer()
        assert self.rec.loadModel(path), fa._lib.last_error()
        self.dim = self.rec.feature_dim()
        self.handle = self.rec._h

    def run(self, frames):
        n = len(frames)
        d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        out = torch.zeros((n, self.dim), device="cuda")
        raw = torch.zeros((n, self.dim), device="cuda")
        fa.lib().fh_timing_enable(1)
        try:
            assert self.rec.embed_aligned_dev(d.data_ptr(), n, out.data_ptr(), raw.data_ptr()) == n
            torch.cuda.synchronize()
            tags = _collect_tags()
        finally:
            fa.lib().fh_timing_enable(0)
        return [raw.cpu().numpy()], tags


DET_SWITCHES = [("winograd=0", "fh_det_set_winograd", (0,), (1,), False), ("halo=0", "fh_det_set_halo_conv", (0,), (1,), False),
                ("fused_front=0", "fh_det_set_fused_front", (0,), (1,), True), ("fused_stem=0", "fh_det_set_fused_stem", (0,), (1,), True)]
REC_SWITCHES = [("winograd=0", "fh_rec_set_winograd", (0,), (1,), False), ("wino_fusion=0", "fh_rec_set_wino_fusion", (0,), (1,), True),
                ("shortcut_fold=0", "fh_rec_set_shortcut_fold", (0,), (1,), True), ("fused_stem=0", "fh_rec_set_fused_stem", (0,), (1,), True)]
CFG = [(f"conv_cfg={c},sk=1", (c, 1)) for c in range(4)] + [("conv_cfg=-1,sk=0", (-1, 0))]


def _small_kernels(ops):
    """The small kernels a plan launches, keyed as in SMALL_KERNELS (the depthwise ones by the form launch_dwconv3x3 picks)."""
    out = {}
    for o in ops:
        k = "DWCONV " + gg.dw_form(o) if o["kind"] == "DWCONV" else o["kind"]
        if k in SMALL_KERNELS:
            out[k] = out.get(k, 0) + 1
    return out


def _exercise(runner, refs, handle, switches, cfg_fn, seed, h, w, ops, spec, ledger):
    bhi = b_hi(ops)
    mid = bhi // 2
    fa_ = _u8(bhi, h, w, seed * 7 + 1)
    f1 = _u8(1, h, w, seed * 7 + 2)
    fc = _u8(bhi, h, w, seed * 7 + 3)
    slots = [0, mid, bhi - 1]
    small = _small_kernels(ops)
    n_other = sum(v for k, v in small.items() if k in ("ACT", "ADD", "AFFINE", "UPSAMPLE", "DWGLOBAL"))
    n_dw = sum(v for k, v in small.items() if k.startswith("DWCONV") or k == "GCONV")

    def step(frames, key, idx, what, rows=None, src=None):
        """Run `frames`; slot rows[k] of the result is image idx[k] of the frame set `key`, `src` (defaults: idx, frames)."""
        got, tags = runner.run(frames)
        ledger["tags"].update(tags)
        rows = idx if rows is None else rows
        _check([g[rows] for g in got], refs.get(frames if src is None else src, key, idx), idx, 7 in tags,
               f"seed {seed} {what} B={len(frames)}", spec)
        assert tags.count(5) >= n_other and tags.count(4) >= n_dw, (what, tags)   # every small op launched its kernel (tags 5 / 4)
        for k, v in small.items():
            ledger["kinds"][k] = ledger["kinds"].get(k, 0) + v
        return got, tags

    step(fa_, "a", slots, "default")
    base1, t1 = step(f1, "b", [0], "default")
    basec, thi = step(fc, "c", slots, "default")
    again, _ = runner.run(fc)
    for x, y in zip(basec, again):
        assert np.array_equal(x, y), f"seed {seed}: a repeated call is not bitwise identical\n{spec}"
    step(fc[slots], "c", slots, "default", rows=[0, 1, 2], src=fc)                  # B = 3: the same images as B_hi's first / middle / last
    # B_hi straddles the batch-dependent forms: more layers switch on than at B = 1, and (when the model says some stay off) fewer than
    # at the next crossing above it — counted as launches of those forms
    dep = lambda tags: sum(tags.count(t) for t in BATCH_FORMS)
    assert dep(thi) >= _on(ops, bhi) and dep(t1) >= _on(ops, 1), f"seed {seed}: a layer missed its batch-dependent form: {t1} / {thi}\n{spec}"
    if _on(ops, bhi) > _on(ops, 1):
        assert dep(thi) > dep(t1), f"seed {seed}: no batch-dependent form switched on between B = 1 and B_hi = {bhi}: {t1} / {thi}\n{spec}"
    above = [c for c in _crossings(ops) if c > bhi]
    if above and _on(ops, above[0]) > _on(ops, bhi):
        _, tnext = runner.run(_u8(above[0], h, w, seed * 7 + 4))
        assert dep(tnext) > dep(thi), f"seed {seed}: B_hi = {bhi} already ran every form that B = {above[0]} runs\n{spec}"
    for what, fn, off, on, fused in switches:
        getattr(fa.lib(), fn)(handle, *off)
        try:
            for frames, key, idx, base in ((fc, "c", slots, basec), (f1, "b", [0], base1)):
                got, _ = step(frames, key, idx, what)
                if fused:
                    for x, y in zip(got, base):
                        scale = max(float(np.abs(x).max()), 1e-6)
                        err = float(np.abs(x[idx] - y[idx]).max())
                        assert err <= 1e-5 * scale, f"seed {seed} {what}: fused vs unfused {err:.3g} of {scale:.3g}\n{spec}"
        finally:
            getattr(fa.lib(), fn)(handle, *on)
    for what, args in CFG:
        cfg_fn(handle, *args)
        try:
            step(fc, "c", slots, what)
            step(f1, "b", [0], what)
        finally:
            cfg_fn(handle, -1, 1)


def _run_graph(seed, d, ledger):
    fa.lib().fh_init(0)
    path, spec = gg.make_graph(seed, d)
    h, w = (int(v) for v in spec.split()[1].split("x"))
    ops = gg.parse_ops(api.plan_describe(path, h, w))
    spec = f"B_hi {b_hi(ops)}  crossings {_crossings(ops)}\n{spec}"
    det = DetRunner(path, h, w)
    refs = Refs(path, True)
    _exercise(det, refs, det.det.handle, DET_SWITCHES, fa.lib().fh_det_set_conv_cfg, seed, h, w, ops, spec, ledger)
    if len(refs.names) == 1:
        rec = RecRunner(path, h, w)
        _exercise(rec, Refs(path, False), rec.handle, REC_SWITCHES, fa.lib().fh_rec_set_conv_cfg, seed, h, w, ops, spec, ledger)
    ledger["graphs"].add(seed)


@pytest.fixture(scope="session")
def ledger():
    """Timing tags and small kernels seen across the corpus, filled by every graph run of the session."""
    return {"tags": set(), "kinds": {}, "graphs": set()}


@pytest.mark.parametrize("seed", SEEDS)
def test_graph_matches_fp64_across_batches_and_switches(tmp_path, seed, ledger):
    assert torch.cuda.is_available(), "GPU tests need a real device: the product path has no CPU fallback"
    _run_graph(seed, str(tmp_path), ledger)


def test_kernel_ledger_reaches_every_tag_and_small_kernel(tmp_path, ledger):
    """Every timing tag occurred across the corpus, and every small kernel that only a synthetic model reaches (act / add / affine /
    upsample2x / dwglobal / gconv3x3, and dwconv3x3 in its lean, generic stride-1 and hstrip stride-2 forms) ran inside a graph that
    matched fp64.  Graphs the session has not run yet (this test selected alone) are run here."""
    assert torch.cuda.is_available(), "GPU tests need a real device: the product path has no CPU fallback"
    for seed in SEEDS:
        if seed not in ledger["graphs"]:
            _run_graph(seed, str(tmp_path), ledger)
    missing_tags = sorted(set(range(TAGS)) - ledger["tags"])
    assert not missing_tags, f"the corpus no longer reaches timing tags {missing_tags}"
    missing = [k for k in SMALL_KERNELS if not ledger["kinds"].get(k)]
    assert not missing, f"the corpus no longer launches {missing}"
