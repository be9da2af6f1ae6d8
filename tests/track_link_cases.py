"""Hand-made clips for the re-linking tests (tests/test_track_link_model_cpu.py, tests/test_gpu_track_link.py): people at fixed places
who vanish for longer than max_missed and come back.  A clip is a list of frames, a frame a list of (place, person); the places are
40 x 40 boxes on a grid of pitch 60, so two places never overlap and the IoU tracker follows a person exactly as long as they stay where they are.
embeddings() turns the persons into rows: EXACT ones (small integers on a few coordinates: every dot product and sum of squares is
exact in fp32 in any order) or seeded random unit rows with a noisy copy per appearance.  Not a test module."""
from __future__ import annotations

import numpy as np

import facerecognizeonnx_amd as fa

MAX_MISSED = 1                                                      # a track is dead once it has missed 2 frames


def box(place):
    return (60 * (place % 40), 60 * (place // 40), 40, 40)


class Clip:
    def __init__(self, frames, per_frame, stream_of=None):
        self.frames, self.n, self.per_frame = frames, len(frames), per_frame
        self.stream_of = None if stream_of is None else np.asarray(stream_of, np.int32)
        self.det = np.zeros((self.n, per_frame), fa.FACE_DTYPE)
        self.counts = np.zeros(self.n, np.int32)
        self.person = np.full((self.n, per_frame), -1, np.int64)
        for f, faces in enumerate(frames):
            assert len(faces) <= per_frame
            self.counts[f] = len(faces)
            for j, (place, who) in enumerate(faces):
                self.det[f, j]["x"], self.det[f, j]["y"], self.det[f, j]["w"], self.det[f, j]["h"] = box(place)
                self.det[f, j]["score"] = 0.9
                self.person[f, j] = who

    def sub(self, a, b):
        return Clip(self.frames[a:b], self.per_frame, None if self.stream_of is None else self.stream_of[a:b])


def exact_rows(persons, dim):
    """Person p = 1.0 on coordinate p (p < dim): same person scores 1.0, another one 0.5, whatever the template's count."""
    rows = np.zeros((len(persons), dim), np.float32)
    rows[np.arange(len(persons)), np.asarray(persons) % dim] = 1.0
    return rows


def random_rows(persons, dim, seed, noise=0.5):
    """Person p = a seeded unit row; every appearance a fresh noisy copy, normalised."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((int(max(persons)) + 1, dim)).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    x = base[np.asarray(persons)] + np.float32(noise / np.sqrt(dim)) * rng.standard_normal((len(persons), dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, np.float32)


def gaps(*visits):
    """frames from (first, last, [(place, person)]) visits (inclusive)."""
    n = max(v[1] for v in visits) + 1
    frames = [[] for _ in range(n)]
    for first, last, faces in visits:
        for f in range(first, last + 1):
            frames[f] += faces
    return frames


A, B, C, D = 1, 2, 3, 4
# name -> (frames, per_frame, max_tracks, memory, max_age, events the model must show)
CLIPS = {
    # A is seen, hidden for four frames and comes back somewhere else: the lowest free slot is its own
    "same_slot": (gaps((0, 2, [(0, A)]), (7, 9, [(5, A)])), 1, 1, 0, 150, {"same_slot"}),
    # B takes A's slot while A is away (A retires to the memory); A comes back into slot 1
    "from_memory": (gaps((0, 2, [(0, A)]), (5, 9, [(1, B)]), (7, 9, [(2, A)])), 5, 3, 1, 150, {"from_memory", "retired", "refused"}),
    "no_memory": (gaps((0, 2, [(0, A)]), (5, 9, [(1, B)]), (7, 9, [(2, A)])), 5, 3, 0, 150, {"dropped_no_memory", "refused"}),
    # B (slot 0) and A (slot 1) both vanish; A comes back alone into slot 0: the winner is another slot's row, B retires
    "other_slot": (gaps((0, 2, [(0, B), (1, A)]), (7, 9, [(2, A)])), 5, 3, 8, 150, {"other_slot", "retired"}),
    # X -> Y -> Z
    "chain": (gaps((0, 1, [(0, A)]), (5, 6, [(1, A)]), (10, 11, [(2, A)])), 1, 1, 1, 150, {"chain", "same_slot"}),
    # two faces of A's open in one frame: the first in j order gets A's lost track
    "competition": (gaps((0, 1, [(0, A)]), (5, 6, [(1, A), (2, A)])), 5, 3, 8, 150, {"same_slot"}),
    # two lost tracks with identical templates: the smaller owner wins
    "twins": (gaps((0, 1, [(0, A), (1, A)]), (5, 6, [(2, A)])), 5, 3, 8, 150, {"tie_smaller_owner"}),
    # max_age: A's last entry is t = 1 and it returns at t = 8: the gap is 6
    "age_in_reach": (gaps((0, 1, [(0, A)]), (8, 9, [(1, A)])), 1, 1, 1, 6, {"same_slot"}),
    "age_beyond": (gaps((0, 1, [(0, A)]), (8, 9, [(1, A)])), 1, 1, 1, 5, set()),
    # one slot, one memory row, four people in turn: the memory evicts by last_seen, so A is forgotten when it returns ...
    "evict": (gaps((0, 1, [(0, A)]), (5, 6, [(1, B)]), (10, 11, [(2, C)]), (15, 16, [(3, A)])), 1, 1, 1, 150, {"evicted", "refused"}),
    # ... and remembered with room for all
    "keep": (gaps((0, 1, [(0, A)]), (5, 6, [(1, B)]), (10, 11, [(2, C)]), (15, 16, [(3, A)])), 1, 1, 8, 150, {"from_memory"}),
    # one slot, two memory rows: A, then B, then A again — resumed from the memory into the slot that B had — then C, which retires the
    # resumed record in its turn
    "resume_retire": (gaps((0, 1, [(0, A)]), (5, 6, [(1, B)]), (10, 11, [(2, A)]), (15, 16, [(3, C)])), 1, 1, 2, 150, {"from_memory", "retired"}),
}
# clips cut into two calls after an earlier call has NAMED the slot: (clip, first frame of the second call, events of the model).  In the
# second call a record is opened (evict: B, then C; resume_retire: B) or resumed (resume_retire: A) and retired again before it ends;
# chain is resumed twice in the slot its first call named.
CUTS = [("evict", 2, {"retired_opened_this_call", "retired_from_a_named_slot"}),
        ("resume_retire", 3, {"retired_opened_this_call", "retired_resumed_this_call", "retired_from_a_named_slot"}),
        ("chain", 2, {"chain", "same_slot"})]


def clip(name):
    frames, per_frame, max_tracks, memory, max_age, events = CLIPS[name]
    return Clip(frames, per_frame), dict(max_tracks=max_tracks, memory=memory, max_age=max_age), events


def crowd(per_frame=70, people=66, seed=5):
    """per_frame 70, max_tracks 64: 66 people (two stay untracked), all hidden for three frames, back at shuffled places."""
    rng = np.random.default_rng(seed)
    first = [(k, 100 + k) for k in range(people)]
    back = [(100 + k, 100 + int(p)) for k, p in enumerate(rng.permutation(people))]
    return Clip(gaps((0, 1, first), (5, 6, back)), per_frame)


def three_streams():
    """Three cameras interleaved, each with its own occlusion (the persons differ per stream, the places do not)."""
    per = [gaps((0, 2, [(0, 10 * s + A), (1, 10 * s + B)]), (6 + s, 9 + s, [(3, 10 * s + A)]), (8 + s, 9 + s, [(4, 10 * s + B)])) for s in range(3)]
    rng = np.random.default_rng(11)
    stream_of = rng.permutation(np.concatenate([np.full(len(p), s) for s, p in enumerate(per)]))
    nxt = [0, 0, 0]
    frames = []
    for s in stream_of:
        frames.append(per[s][nxt[s]])
        nxt[s] += 1
    return Clip(frames, 5, stream_of)
