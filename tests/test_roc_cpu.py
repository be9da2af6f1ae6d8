"""The bin rule and the ROC read-out on the host (fh_hist_bin, fh_roc_from_hist, csrc/roc_plan.h) against the Python-int model of
tests/roc_model.py: every fp32 bin edge and its neighbours, the clamps, NaN; the suffix-sum property that ties a histogram to the
library's strict test `score > threshold`; seeded random histograms up to the 128-bit path; plateaus, exact k / N_i budgets, the
no-solution point, empty planes and bad arguments.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import roc_model as rm

FH_ERR_ARG, FH_ERR_STATE = -1, -4
BINS = rm.BINS
F = np.float32


def got_bins(values):
    L = _lib.lib()
    return np.array([L.fh_hist_bin(float(v)) for v in np.asarray(values, F)], np.int64)


def check_bins(values):
    values = np.asarray(values, F)
    got, want = got_bins(values), rm.bins(values)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (values[bad[:8]], got[bad[:8]], want[bad[:8]])
    return got


def test_the_constant_and_the_python_wrapper():
    assert fa.HIST_BINS == BINS == 2048
    assert fa.hist_bin(0.6) == rm.bin_of(F(0.6)) == 1228 and fa.hist_bin(float("nan")) == -1


def test_every_edge_and_its_two_neighbours():
    edges = (np.arange(0, BINS + 1, dtype=np.float64) / BINS).astype(F)
    assert np.array_equal(edges.astype(np.float64) * BINS, np.arange(0, BINS + 1))            # b/2048 is an exact fp32 value
    below, above = np.nextafter(edges, F(-1)), np.nextafter(edges, F(2))
    got = check_bins(np.concatenate([edges, below, above]))
    at, lo, hi = got[:BINS + 1], got[BINS + 1:2 * BINS + 2], got[2 * BINS + 2:]
    b = np.arange(1, BINS)
    assert np.array_equal(at[b], b - 1) and np.array_equal(lo[b], b - 1) and np.array_equal(hi[b], b)   # an edge belongs to the bin below it
    assert at[0] == lo[0] == hi[0] == 0 and at[BINS] == lo[BINS] == hi[BINS] == BINS - 1


def test_clamps_zeros_denormals_and_nan():
    tiny = np.finfo(F).tiny
    vals = [0.0, -0.0, -1e-30, -0.25, -1.0, -3e38, -np.inf, 1e-45, -1e-45, tiny, -tiny, tiny / 4, 1.0 / 4096, 1.0,
            np.nextafter(F(1), F(2)), 1.5, 2.0, 3e38, np.inf]
    got = check_bins(vals)
    assert (got[:13] == 0).all() and (got[13:] == BINS - 1).all()
    assert got_bins([np.nan, -np.nan]).tolist() == [-1, -1] and rm.bins([np.nan]).tolist() == [-1]


def test_random_floats():
    rng = np.random.default_rng(1)
    check_bins(rng.random(60000, dtype=F) * F(1.2) - F(0.1))
    bits = rng.integers(0, 1 << 32, 40000, dtype=np.uint64).astype(np.uint32)     # any bit pattern: huge, tiny, negative, NaN, inf
    check_bins(bits.view(F))


def test_a_suffix_sum_is_the_count_of_the_strict_test():
    rng = np.random.default_rng(2)
    for n, lo, hi in ((5000, -0.05, 1.05), (3000, 0.45, 0.55), (64, 0.0, 1.0)):
        s = (rng.random(n, dtype=F) * F(hi - lo) + F(lo)).astype(F)
        s[: n // 8] = (rng.integers(0, BINS + 1, n // 8) / BINS).astype(F)          # a good share sits exactly on edges
        b = got_bins(s)
        h = np.bincount(b, minlength=BINS)
        suffix = np.cumsum(h[::-1])[::-1]
        for t in range(1, BINS):
            assert suffix[t] == int((s > F(t / BINS)).sum()), t
        assert suffix[0] == n


def c_roc(hist, max_far, sentinel=0x5A):
    out = np.full(2 * _lib.ROC_POINT_DTYPE.itemsize + 16, sentinel, np.uint8)
    hist = np.ascontiguousarray(hist, np.uint64)
    rc = _lib.lib().fh_roc_from_hist(hist.ctypes.data, C.c_double(max_far), out.ctypes.data)
    assert (out[-16:] == sentinel).all()
    return rc, out[:-16].view(_lib.ROC_POINT_DTYPE), out


def both(hist, max_far):
    want = rm.roc(hist, max_far)
    assert want is not None
    rc, got, _ = c_roc(hist, max_far)
    assert rc == 0
    for k in range(2):
        g = (got[k]["threshold"], int(got[k]["bin"]), int(got[k]["true_accepts"]), int(got[k]["false_accepts"]), int(got[k]["genuine"]),
             int(got[k]["impostor"]))
        assert g[0].view(np.uint32) == want[k][0].view(np.uint32) and g[1:] == want[k][1:], (k, max_far, g, want[k])
    return want


def bell(rng, centre, width, total):
    """a histogram plane: `total` counts spread over a bump of bins (Python ints, so that totals near 2^62 stay exact)"""
    w = np.exp(-0.5 * ((np.arange(BINS) - centre) / width) ** 2) * rng.random(BINS)
    w[w < 1e-6] = 0.0                                             # zero tails: plateaus of A on both sides
    share = [int(x * (1 << 40)) for x in w]
    tot = sum(share)
    out = [x * total // tot for x in share]
    out[int(np.argmax(w))] += total - sum(out)                    # the rounding's remainder: the plane sums to `total` exactly
    return np.array(out, np.uint64)


@pytest.mark.parametrize("scale", [1000, 10 ** 7, 3 * 2 ** 32, 2 ** 48, 2 ** 62])
def test_random_histograms(scale):
    rng = np.random.default_rng(scale % 9973)
    for rep in range(6):
        n_i = scale - int(rng.integers(0, 500))
        n_g = max(scale // int(rng.integers(1, 50)), 7)
        hist = np.stack([bell(rng, rng.integers(1300, 2000), rng.integers(20, 200), n_g),
                         bell(rng, rng.integers(900, 1400), rng.integers(10, 150), n_i)])
        n_i = sum(int(x) for x in hist[1])
        for max_far in (0.0, 1.0, 1e-6, 1e-4, 0.01, 0.5, float(rng.random()), 3 / n_i, (n_i // 7) / n_i, (n_i - 1) / n_i):
            both(hist, max_far)


def test_a_budget_of_exactly_k_over_n():
    hist = np.zeros((2, BINS), np.uint64)
    hist[0, 1800] = 50
    hist[1, 1000:1010] = 100                                      # N_i = 1000; A_i drops by 100 per bin
    for k in (0, 100, 199, 200, 201, 999, 1000):
        op, _ = both(hist, k / 1000)
        assert op[3] == (k // 100) * 100 and op[1] == (1 if k == 1000 else 1010 - k // 100)
    assert both(hist, 0.0)[0][1:4] == (1010, 50, 0)               # the smallest threshold that accepts no impostor keeps every genuine pair


def test_on_a_plateau_the_smallest_bin_wins():
    hist = np.zeros((2, BINS), np.uint64)
    hist[0, 1500], hist[0, 1900] = 30, 70
    hist[1, 200], hist[1, 900] = 1000, 10                         # A_i = 10 on bins 201..900, 0 above
    op, eer = both(hist, 0.01)
    assert op[1] == 201 and op[2:4] == (100, 10)
    assert both(hist, 0.0)[0][1] == 901
    assert eer[1] == 901                                          # FAR 10/1010 > FRR 0 on 201..900; FAR 0 <= FRR 0 from 901 on
    hist[1, 900] = 0
    hist[1, 200] = 1010
    assert both(hist, 0.5)[1][1] == 201                           # FAR 0 <= FRR 0 from bin 201 on: the first of a long plateau


def test_no_solution_gives_bin_minus_one():
    hist = np.zeros((2, BINS), np.uint64)
    hist[0, 5], hist[0, BINS - 1], hist[1, BINS - 1] = 8, 1, 4    # every impostor in the top bin: FAR = 1 everywhere, FRR < 1 up there
    op, eer = both(hist, 0.0)
    assert op == (F(1.0), -1, 0, 0, 9, 4) and eer == (F(1.0), -1, 0, 0, 9, 4)
    assert both(hist, 1.0)[0][1] == 1                             # a budget of everything: the lowest threshold
    p0, p1 = fa.roc_from_hist(hist, 0.0)
    assert p0["bin"] == -1 and p0["threshold"] == 1.0 and p0["far"] == 0.0 and p0["tar"] == 0.0 and p1["bin"] == -1


def test_the_python_wrapper_returns_the_fields_and_the_rates():
    hist = np.zeros((2, BINS), np.uint64)
    hist[0, 1500], hist[0, 1900] = 30, 70
    hist[1, 200], hist[1, 1600] = 990, 10
    op, eer = fa.roc_from_hist(hist, 0.0)
    assert op == {"threshold": 1601 / 2048, "bin": 1601, "true_accepts": 70, "false_accepts": 0, "genuine": 100, "impostor": 1000,
                  "far": 0.0, "tar": 0.7}
    want = rm.roc(hist, 0.0)[1]
    assert (eer["bin"], eer["true_accepts"], eer["false_accepts"]) == want[1:4] and eer["far"] == want[3] / 1000
    with pytest.raises(ValueError):
        fa.roc_from_hist(hist[:, :100], 0.1)


def test_errors_write_nothing():
    L = _lib.lib()
    hist = np.zeros((2, BINS), np.uint64)
    hist[0, 1500], hist[1, 700] = 3, 5
    out = np.full(96, 0x5A, np.uint8)
    for far in (-1e-9, 1.0000001, float("nan"), float("inf"), -float("inf")):
        rc, _, raw = c_roc(hist, far)
        assert rc == FH_ERR_ARG and (raw == 0x5A).all() and rm.roc(hist, far) is None and _lib.last_error()
    assert L.fh_roc_from_hist(None, C.c_double(0.1), out.ctypes.data) == FH_ERR_ARG and (out == 0x5A).all()
    assert L.fh_roc_from_hist(hist.ctypes.data, C.c_double(0.1), None) == FH_ERR_ARG
    for plane in (0, 1):
        h = hist.copy()
        h[plane] = 0
        rc, _, raw = c_roc(h, 0.1)
        assert rc == FH_ERR_STATE and (raw == 0x5A).all() and rm.roc(h, 0.1) is None and _lib.last_error()
    with pytest.raises(_lib.FaceHipError):
        fa.roc_from_hist(np.zeros((2, BINS), np.uint64), 0.1)
    assert c_roc(hist, 0.1)[0] == 0
