"""A watchlist per camera on the GPU (fh_tracker_set_stream_masks): fh_track_identify_dev called directly with synthetic embeddings, its
labels and scores held BIT FOR BIT to tests/track_tags_model.py — tests/track_ident_model.py with a stage B built on the tags model,
given the device's own queries.  Two streams see the same faces; the gallery holds identity 11 (tag bit 0) and identity 22 (tag bit 1);
the stream masks are {1, 2}."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import gallery_fuse_model as gm    # noqa: E402
from tests import gallery_tags_model as tags_model  # noqa: E402
from tests import track_ident_model as im     # noqa: E402
from tests import track_tags_model as ttm     # noqa: E402

DIM, THR, BASE = 64, 0.6, 40
N, PER = 12, 2                                                     # frames (streams alternate), faces per frame
KW = dict(streams=2, max_tracks=1, iou_thr=0.3, max_missed=0, refresh=2)
STREAM_OF = np.arange(N, dtype=np.int32) % 2
ID_A, ID_B = 11, 22


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def from_device(ptr, shape, dtype=np.float32):
    out = np.empty(shape, dtype)
    if out.size:
        assert ptr and fa.lib().fh_memcpy_d2h(out.ctypes.data, ptr, out.nbytes) == 0, _lib.last_error()
    return out


def unit(x):
    x = np.asarray(x, np.float32)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


class World:
    """The gallery (two templates per identity among a few strangers), the detections and one embedding per entry."""

    def __init__(self, labelled, both_above):
        rng = np.random.default_rng(77)
        a, b = unit(rng.standard_normal(DIM)), unit(rng.standard_normal(DIM))
        noise = lambda: np.float32(0.1) * unit(rng.standard_normal(DIM))                 # noqa: E731
        self.rows = np.ascontiguousarray(np.stack([unit(rng.standard_normal(DIM)), unit(a + noise()), unit(b + noise()),
                                                   unit(rng.standard_normal(DIM)), unit(b + noise()), unit(a + noise())]), np.float32)
        self.ids = np.array([5, ID_A, ID_B, 6, ID_B, ID_A], np.int32) if labelled else None
        self.tags = np.array([4, 1, 2, 4, 2, 1], np.uint32)
        self.a_rows, self.b_rows = [1, 5], [2, 4]
        self.g = fa.Gallery(DIM)
        rd = dev(self.rows)
        if labelled:
            self.g.upload(rd.data_ptr(), 6, True, BASE, ids_ptr=dev(self.ids).data_ptr())
        else:
            self.g.upload(rd.data_ptr(), 6, True, BASE)
        self.g.set_tags(self.tags)
        # face 0 of every frame sits in one place (one track per stream); face 1 finds no free slot: untracked (slot -1), embedded every frame
        self.det = np.zeros((N, PER), fa.FACE_DTYPE)
        self.det["w"], self.det["h"], self.det["score"] = 50, 50, 0.9
        self.det["x"][:, 0], self.det["y"][:, 0] = 10, 10
        self.det["x"][:, 1], self.det["y"][:, 1] = 300, 200
        self.counts = np.full(N, PER, np.int32)
        # the tracked face: mostly B with (both_above) enough of A that A too scores above the threshold; the untracked one: B alone
        mix = np.float32(0.55 if both_above else 0.0)
        self.emb = np.empty((N, PER, DIM), np.float32)
        for f in range(N):
            self.emb[f, 0] = unit(np.float32(0.8) * b + mix * a + noise())
            self.emb[f, 1] = unit(b + noise())
        # and at the end somebody nobody knows: orthogonal to every gallery row (to rounding), so every score is 0.5 < THR
        basis = np.linalg.qr(self.rows.astype(np.float64).T)[0]
        x = rng.standard_normal((2, DIM))
        self.emb[N - 2:, 1] = unit(x - (x @ basis) @ basis.T)

    def name(self, row):
        return self.ids[row] if self.ids is not None else BASE + row


def run(trk, w, masks_model=None):
    """update + identify over all frames; returns the device outputs and, with masks_model = (model, stream masks), what it wants."""
    i32 = lambda v: torch.full((N, PER), v, dtype=torch.int32, device="cuda")              # noqa: E731
    d = dev(np.ascontiguousarray(w.det).view(np.uint8).reshape(-1, 60))
    cnt = dev(w.counts)
    track, embed, slot, label = i32(77), i32(77), i32(77), i32(77)
    score = torch.full((N, PER), 7.0, device="cuda")
    assert trk.update_dev(d.data_ptr(), cnt.data_ptr(), N, PER, track.data_ptr(), embed.data_ptr(), stream_of=STREAM_OF,
                          slot_ptr=slot.data_ptr()) == N
    torch.cuda.synchronize()
    e = embed.cpu().numpy()
    rows = np.ascontiguousarray(w.emb[e != 0])
    total = len(rows)
    d_emb = dev(rows)
    assert trk.identify_dev(w.g, THR, track.data_ptr(), slot.data_ptr(), embed.data_ptr(), d_emb.data_ptr(), total, N, PER,
                            label.data_ptr(), score.data_ptr(), stream_of=STREAM_OF) == N
    torch.cuda.synchronize()
    out = dict(track=track.cpu().numpy(), embed=e, slot=slot.cpu().numpy(), label=label.cpu().numpy(), score=score.cpu().numpy(),
               total=total, queries=from_device(trk.queries_ptr(), (total, DIM)))
    if masks_model is not None:
        model, smasks = masks_model
        wt, we, ws = model.update(w.det, w.counts, PER, STREAM_OF)
        for key, want in (("track", wt), ("embed", we), ("slot", ws)):
            assert np.array_equal(out[key], want), key
        want_l, want_s, q64, verbatim, qm = ttm.identify(model, wt, ws, we, rows, w.rows, w.tags, smasks, THR, w.ids, BASE,
                                                         stream_of=STREAM_OF, queries=out["queries"])
        assert out["queries"][verbatim].tobytes() == rows[verbatim].tobytes()
        assert gm.within_unit_tolerance(out["queries"][~verbatim], q64[~verbatim], DIM).all()
        out.update(want_l=want_l, want_s=want_s, qm=qm)
    return out


def make():
    trk = fa.Tracker(**KW)
    trk.enable_identity(DIM, im.POOL_SUM)
    return trk, im.IdentTracker(DIM, im.POOL_SUM, **KW)


@pytest.mark.parametrize("labelled", [True, False])
@pytest.mark.parametrize("both_above", [False, True])
def test_every_stream_names_faces_from_its_own_watchlist(labelled, both_above):
    w = World(labelled, both_above)
    trk, model = make()
    trk.set_stream_masks([1, 2])
    out = run(trk, w, (model, [1, 2]))
    assert np.array_equal(out["qm"], np.where(np.repeat(STREAM_OF, PER).reshape(N, PER)[out["embed"] != 0] == 0, 1, 2))
    assert np.array_equal(out["label"], out["want_l"]), np.argwhere(out["label"] != out["want_l"])[:5]
    assert out["score"].tobytes() == out["want_s"].tobytes()
    lab, s0, s1 = out["label"], STREAM_OF == 0, STREAM_OF == 1
    # stream 1 (mask 2) names the face B, flagged frames and carried ones alike
    assert np.isin(lab[s1, 0], [w.name(r) for r in w.b_rows]).all()
    assert np.isin(lab[s1, 1][:-1], [w.name(r) for r in w.b_rows]).all() and lab[s1, 1][-1] == -1
    # stream 0 (mask 1) sees the same embeddings but only the rows of A: A where A is above the threshold, nobody otherwise
    if both_above:
        assert np.isin(lab[s0, 0], [w.name(r) for r in w.a_rows]).all()
    else:
        assert (lab[s0, 0] == -1).all() and (out["score"][s0, 0] > 0).all() and (out["score"][s0, 0] <= THR).all()
    assert (lab[s0, 1] == -1).all()                                  # the untracked faces carry their stream's mask too
    assert {"untracked", "pooled"} <= model.events and (not both_above or "carried" in model.events)
    assert (out["embed"][:, 0] == 0).any() and (out["slot"][:, 1] == -1).all()
    # the untagged answer names B on both streams: the masks made the difference
    plain, _ = make()
    ref = run(plain, w)
    assert np.isin(ref["label"][s0, 0], [w.name(r) for r in w.b_rows]).all()


def test_masks_off_is_bit_for_bit_a_tracker_that_never_had_masks():
    w = World(True, True)
    never, _ = make()
    ref = run(never, w)
    trk, _ = make()
    trk.set_stream_masks([1, 2])
    trk.set_stream_masks(None)
    w.g.tag_stats()
    off = run(trk, w)
    assert w.g.tag_stats() == (0, 0)                                 # no tagged scan ran
    for key in ("track", "embed", "slot", "label", "score", "queries"):
        assert off[key].tobytes() == ref[key].tobytes(), key
    for s in (0, 1):
        for a, b in zip(trk.identity(s, sums=True), never.identity(s, sums=True)):
            assert a.tobytes() == b.tobytes()
    # all-ones masks on rows that all carry a tag: the same answer through the tagged call
    ones, _ = make()
    ones.set_stream_masks([tags_model.TAG_ALL, tags_model.TAG_ALL])
    on = run(ones, w)
    assert w.g.tag_stats()[0] > 0
    for key in ("label", "score"):
        assert on[key].tobytes() == ref[key].tobytes(), key


def test_argument_errors():
    L = fa.lib()
    assert L.fh_tracker_set_stream_masks(None, None) == -1
    trk, _ = make()
    with pytest.raises(ValueError):
        trk.set_stream_masks([1, 2, 3])
