"""Seeded random ONNX graphs (tests/graphgen.py) through the planner, without a GPU.

* every corpus graph plans; every graph just outside the vocabulary is refused cleanly (plan_describe raises, loadModel is false,
  fh_last_error() says why);
* the arena checker: for every op of every plan — the corpus and the synthetic models — the tensors it touches, the implied reads of
  the bn<-op / sc<-op links included, are live at that op, and tensors whose lifetimes meet occupy disjoint floats;
* the oracle agrees with the torch fp64 evaluation of every graph (the 2e-5-of-scale bar of test_exported_onnx.py), so that the GPU
  tests can lean on it for these combinations;
* the plan ledger: each op kind and annotation of describe() occurs at least twice across the corpus.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import api
from facerecognizeonnx_amd.synth import models
from oracle import onnx_min, oracle
from oracle import torch_graph as torch_ref
from tests import graphgen as gg
from tests import util

TENSOR_RE = re.compile(r"tensor t(\d+) (\d+)x(\d+)x(\d+) off (\d+) live (-?\d+)\.\.(-?\d+)")
parse_ops = gg.parse_ops


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("graphs"))
    return {s: gg.make_graph(s, d) for s in gg.ALL_SEEDS}


def check_arena(desc):
    """Every access inside its tensor's live interval; tensors whose intervals meet never share a float."""
    ops = parse_ops(desc)
    tens = {int(m.group(1)): (int(m.group(2)) * int(m.group(3)) * int(m.group(4)), int(m.group(5)), int(m.group(6)), int(m.group(7)))
            for m in TENSOR_RE.finditer(desc)}
    assert ops and tens
    for o in ops:
        acc = o["reads"] + o["writes"]
        if o["bn"] >= 0:                                    # the consumer may read the producer's PLAIN output at its own position
            acc.append(ops[o["bn"]]["out"])
        if o["sc"] >= 0:                                    # the folded shortcut reads the shortcut conv's input at this op
            acc.append(ops[o["sc"]]["reads"][0])
        for t in acc:
            assert t in tens, (o["text"], t)
            first, last = tens[t][2], tens[t][3]
            assert first <= o["i"] <= last, f"op {o['i']} touches t{t} outside its lifetime {first}..{last}: {o['text']}"
    items = sorted(tens.items())
    for a, (ea, oa, fa_, la) in items:
        for b, (eb, ob, fb, lb) in items:
            if a < b and not (la < fb or lb < fa_):
                assert oa + ea <= ob or ob + eb <= oa, f"t{a} [{oa},{oa + ea}) live {fa_}..{la} overlaps t{b} [{ob},{ob + eb}) live {fb}..{lb}"
    return ops


def test_every_corpus_graph_plans_and_its_arena_is_sound(corpus):
    for seed, (path, spec) in corpus.items():
        h, w = (int(v) for v in spec.split()[1].split("x"))
        try:
            desc = api.plan_describe(path, h, w)
            check_arena(desc)
        except Exception as e:
            raise AssertionError(f"seed {seed}: {e}\n{spec}") from e


# the planner's own words for each refusal (plan.cpp fail() messages): a reject must be refused by the check it is named after
REJECT_REASON = {
    "dilation": "dilation != 1",
    "auto_pad": "auto_pad not supported",
    "resize_x3": "Resize: only x2 nearest supported",
    "resize_linear": "Resize: only nearest supported",
    "broadcast_add": "Add operands differ in shape (broadcast unsupported)",
    "grouped_c6": "grouped Conv needs C % 4 == 0",
    "reshape_nchw": "would need a physical transpose",
    "conv5x5": "only 3x3/p1 and 1x1/p0 convolutions are supported",
    "nchw_output": "is NCHW-ordered",
    "maxpool": "unsupported operator 'MaxPool'",
    "const_minus_tensor": "Sub of a constant by a tensor is not supported",
}


@pytest.mark.parametrize("name", sorted(gg.REJECTS))
def test_graphs_outside_the_vocabulary_are_refused_cleanly(tmp_path, name):
    assert set(REJECT_REASON) == set(gg.REJECTS)
    reason = REJECT_REASON[name]
    path = gg.make_reject(name, str(tmp_path))
    with pytest.raises(fa.FaceHipError) as e:
        api.plan_describe(path, 20, 24)
    assert reason in str(e.value), str(e.value)
    for cls in (fa.FaceDetector, fa.FaceRecognizer):
        with pytest.raises(fa.FaceHipError):                       # leave a different message behind first
            api.plan_describe(str(tmp_path / "missing.onnx"), 20, 24)
        assert reason not in fa._lib.last_error()
        h = cls()
        assert not h.loadModel(path)
        assert reason in fa._lib.last_error(), (cls.__name__, fa._lib.last_error())


def _synthetic_models(d):
    yield "r_tiny", util.tiny_iresnet(d), 112, 112
    yield "r_tiny_unfolded", util.tiny_iresnet(d, fold_bn=False), 112, 112
    yield "mbf_tiny", util.tiny_mbf(d), 112, 112
    yield "mbf_tiny_unfolded", util.tiny_mbf(d, fold_bn=False), 112, 112
    yield "scrfd_tiny", util.tiny_scrfd(d), 160, 128
    yield "scrfd_tiny_640", util.tiny_scrfd(d), 640, 640
    for ds in (False, True):
        yield f"r_ds{int(ds)}", models.make_iresnet(f"{d}/ds{int(ds)}.onnx", (1, 2, 1, 1), (32, 64, 128, 128), 112, 64, seed=9,
                                                    downsample_first=ds), 112, 112
    yield "r50", models.cached("w600k_r50_seed200.onnx", models.make_w600k_r50), 112, 112
    yield "mbf", models.cached("w600k_mbf_seed300.onnx", models.make_w600k_mbf), 112, 112
    yield "det_500m", models.cached("det_500m_seed100.onnx", models.make_det_500m), 640, 640
    for name in ("exported_iresnet_default", "exported_iresnet_trained", "exported_scrfd"):
        yield name, f"{util.GOLDEN}/{name}.onnx", 96 if "scrfd" in name else 112, 128 if "scrfd" in name else 112


def test_arena_checker_on_every_synthetic_model(models_dir):
    seen = 0
    for name, path, h, w in _synthetic_models(models_dir):
        try:
            check_arena(api.plan_describe(path, h, w))
        except Exception as e:
            raise AssertionError(f"{name}: {e}") from e
        seen += 1
    assert seen >= 12


def _scale(y):
    return max(float(np.abs(y).max()), 1e-6)


@pytest.mark.parametrize("seed", gg.ALL_SEEDS)
def test_oracle_matches_torch_fp64(corpus, seed):
    path, spec = corpus[seed]
    g = onnx_min.load(path)
    h, w = (int(v) for v in spec.split()[1].split("x"))
    x = np.random.default_rng(seed + 77).uniform(-1, 1, (1, 3, h, w)).astype(np.float32)
    got = oracle.run_graph(g, {"input": x})
    ref = torch_ref.run_graph(g, {"input": x})
    for name, _ in g.outputs:
        r = np.asarray(ref[name])
        o = np.asarray(got[name]).reshape(r.shape)
        err = float(np.abs(o - r).max())
        assert err < 2e-5 * _scale(r), f"seed {seed} output {name}: {err} vs scale {_scale(r)}\n{spec}"


LEDGER = {
    "op kinds": ["CONV", "DWCONV", "GEMM", "AFFINE", "ACT", "ADD", "UPSAMPLE", "DW+PW s1", "DW+PW s2", "DWGLOBAL", "GCONV"],
    "depthwise forms": ["DWCONV lean s1", "DWCONV lean s2", "DWCONV generic s1", "DWCONV generic s2"],
    "activations": ["+relu", "+prelu", "+sigmoid"],
    "residuals": ["+res", "+res(up2x)"],
    "BN second output": ["+bn2nd", "bn2nd-only"],
    "links": ["bn<-op", "sc<-op"],
    "merges": ["[merged x2]", "[merged x3]"],
}


def plan_ledger(descs):
    count = {e: 0 for g in LEDGER.values() for e in g}
    for desc in descs:
        for o in parse_ops(desc):
            count[o["kind"]] = count.get(o["kind"], 0) + 1
            if o["kind"] == "DWCONV":
                count["DWCONV " + gg.dw_form(o)] += 1
            rest = o["text"].split(" -> ", 1)[1]
            for e in LEDGER["activations"] + LEDGER["BN second output"] + LEDGER["links"] + LEDGER["merges"] + ["+res(up2x)"]:
                count[e] += e in rest
            count["+res"] += re.search(r"\+res(?!\()", rest) is not None
    return count


def test_plan_ledger_reaches_every_rule(corpus):
    descs = []
    for seed, (path, spec) in corpus.items():
        h, w = (int(v) for v in spec.split()[1].split("x"))
        descs.append(api.plan_describe(path, h, w))
    count = plan_ledger(descs)
    missing = {e: count[e] for g in LEDGER.values() for e in g if count[e] < 2}
    assert not missing, f"the corpus no longer reaches: {missing}\n{count}"
