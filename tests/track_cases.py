"""The synthetic record streams of the tracker tests (tests/test_gpu_track.py; their hazards are also checked without a GPU in
tests/test_track_model_cpu.py): seeded random walks of integer boxes with births and deaths, one population per camera stream, plus
planted frames — an exact iou tie between two tracks, zero-width and zero-height boxes, a count of 0, a negative count, a count above
per_frame.  Not a test module."""
from __future__ import annotations

import numpy as np

import facerecognizeonnx_amd as fa

# the tie triple: LEFT and RIGHT do not overlap, MID overlaps both by exactly a third — far away from the walkers
FAR = 5000
LEFT, RIGHT, MID = (FAR, FAR, 20, 10), (FAR + 20, FAR, 20, 10), (FAR + 10, FAR, 20, 10)
FLAT, THIN = (FAR + 300, FAR, 0, 9), (FAR + 300, FAR, 9, 0)

# name -> (streams, n, per_frame, max_tracks, max_missed, refresh, events the model's run must show)
CASES = {
    "one_stream": (1, 40, 5, 8, 2, 0, {"tie", "nan", "empty", "negative", "expired", "contest"}),
    "three_streams_exhausted": (3, 60, 5, 4, 0, 3, {"tie", "nan", "empty", "negative", "expired", "exhausted", "refresh"}),
    "64_streams_one_slot": (64, 130, 1, 1, 1, 1, {"nan", "empty", "negative", "expired", "exhausted", "refresh"}),
    "more_faces_than_lanes": (1, 12, 70, 64, 1, 0, {"tie", "nan", "empty", "negative", "overfull", "exhausted", "expired"}),
}
UNUSED_STREAM = 37                                                 # of the 64-stream case
IOU_THRS = (0.3, 0.0)


class Case:
    """stream_of [n], counts [n] (as the detector would write them: may exceed per_frame, planted ones are 0 or negative) and det
    [n][per_frame] FACE_DTYPE records; the entries at and beyond a frame's count hold live-looking garbage that must not be read."""

    def __init__(self, name):
        self.name = name
        self.streams, self.n, self.per_frame, self.max_tracks, self.max_missed, self.refresh, self.events = CASES[name]
        rng = np.random.default_rng(sum(name.encode()))
        self.stream_of = self._stream_of(rng)
        local = np.zeros(self.streams, np.int64)                   # frames of each stream so far
        walkers = [[] for _ in range(self.streams)]
        self.counts = np.zeros(self.n, np.int32)
        self.det = np.zeros((self.n, self.per_frame), fa.FACE_DTYPE)
        for f in range(self.n):
            s = int(self.stream_of[f])
            count, boxes = self._frame(rng, s, int(local[s]), walkers[s])
            local[s] += 1
            self.counts[f] = count
            boxes = boxes[:self.per_frame]
            while len(boxes) < self.per_frame:                     # garbage behind the count: copies of boxes that WOULD match
                boxes.append(boxes[int(rng.integers(len(boxes)))] if boxes and rng.random() < 0.7 else MID)
            for j, b in enumerate(boxes):
                self.det[f, j]["x"], self.det[f, j]["y"], self.det[f, j]["w"], self.det[f, j]["h"] = b
            self.det[f]["score"] = np.sort(rng.uniform(0.5, 1.0, self.per_frame).astype(np.float32))[::-1]
            self.det[f]["lm"] = rng.uniform(0, 600, (self.per_frame, 10)).astype(np.float32)
        self.counts.setflags(write=False)
        self.det.setflags(write=False)

    def _stream_of(self, rng):
        if self.streams == 1:
            return np.zeros(self.n, np.int32)
        if self.streams == 3:
            return rng.permutation(np.repeat(np.arange(3), self.n // 3)).astype(np.int32)
        others = np.array([s for s in range(1, self.streams) if s != UNUSED_STREAM])
        so = np.concatenate([np.zeros(20, np.int64), rng.choice(others, self.n - 20)])     # stream 0 is long enough for the plants
        return rng.permutation(so).astype(np.int32)

    def _walk(self, rng, walkers, cap):
        """One time step of a stream's population: deaths, a drift of a few pixels, births; returns the boxes in a random order."""
        walkers[:] = [w for w in walkers if rng.random() > 0.12]
        for w in walkers:
            w[0] += int(rng.integers(-3, 4)); w[1] += int(rng.integers(-3, 4))
            w[2] = max(8, w[2] + int(rng.integers(-1, 2))); w[3] = max(8, w[3] + int(rng.integers(-1, 2)))
        while len(walkers) < cap and rng.random() < 0.45:
            walkers.append([int(rng.integers(0, 400)), int(rng.integers(0, 400)), int(rng.integers(20, 60)), int(rng.integers(20, 60))])
        return [tuple(walkers[i]) for i in rng.permutation(len(walkers))]

    def _frame(self, rng, s, k, walkers):
        """(count, boxes) of stream s's k-th frame."""
        if self.name == "more_faces_than_lanes":
            cells = [(45 * (i % 10) + int(rng.integers(-2, 3)), 45 * (i // 10) + int(rng.integers(-2, 3)), 30, 30) for i in range(90)]
            count = [70, 90, 66, 70, 64, 0, -1, 3, 70, 65, 69, 70][k]       # (two empty frames: the tie's tracks find free slots)
            if k == 7:
                return 3, [RIGHT, LEFT, FLAT]
            pick = [cells[i] for i in rng.permutation(90)[:max(count, 0)]]
            if k == 8:
                pick[0], pick[1] = MID, THIN                       # MID: a tie between the tracks of RIGHT and LEFT; THIN: 0 / 0 with FLAT's
            return count, pick
        if self.name == "64_streams_one_slot":
            if s == 0:
                plant = {3: (0, []), 4: (1, [FLAT]), 5: (1, [FLAT]), 6: (-4, [(10, 10, 30, 30)]), 7: (1, [THIN]), 8: (3, [(10, 10, 30, 30)])}
                if k in plant:
                    return plant[k]
            boxes = self._walk(rng, walkers, 1)
            extra = int(rng.random() < 0.2)                        # now and then the detector saw one more face than is stored
            return len(boxes) + (extra if boxes else 0), boxes
        # the two 5-per-frame cases: an empty frame first, so that the planted tracks find free slots whatever max_missed is
        plant = {10: (0, []), 11: (0, []), 12: (0, []), 13: (2, [RIGHT, LEFT]), 14: (1, [MID]), 15: (-2, [LEFT, RIGHT]), 16: (1, [FLAT]),
                 17: (2, [FLAT, THIN])}
        if s == 0 and k in plant:
            return plant[k]
        boxes = self._walk(rng, walkers, 5)
        return len(boxes), boxes

    def slices(self, sizes):
        """The batch cut into consecutive calls of the given sizes: [(first, last)]."""
        edges = np.concatenate([[0], np.cumsum(sizes)])
        assert edges[-1] == self.n
        return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
