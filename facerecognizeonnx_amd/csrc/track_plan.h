// track_plan.h — the ONE definition of the order in which the tracker walks a batch (fh_track_plan, and through it fh_track_update_dev):
// a stable counting sort of the frame indices by stream.  Host code, no GPU, no HIP header.
//   order[n]            frame indices grouped by stream, ascending within a stream (batch order = time order)
//   starts[streams + 1] stream s owns order[starts[s] .. starts[s + 1])
// stream_of == nullptr puts every frame on stream 0.  Returns 0, or -1 for n < 1, n > 4096, streams < 1, streams > 4096 or a stream
// index outside [0, streams) — nothing is written then.
#pragma once

namespace fh {

constexpr int kTrackMaxFrames = 4096, kTrackMaxStreams = 4096;

inline int track_plan(const int* stream_of, int n, int streams, int* order, int* starts) {
    if (n < 1 || n > kTrackMaxFrames || streams < 1 || streams > kTrackMaxStreams) return -1;
    if (stream_of)
        for (int f = 0; f < n; ++f)
            if (stream_of[f] < 0 || stream_of[f] >= streams) return -1;
    for (int s = 0; s <= streams; ++s) starts[s] = 0;
    for (int f = 0; f < n; ++f) ++starts[(stream_of ? stream_of[f] : 0) + 1];
    for (int s = 0; s < streams; ++s) starts[s + 1] += starts[s];
    // starts[s] doubles as stream s's write cursor and is wound back afterwards
    for (int f = 0; f < n; ++f) order[starts[stream_of ? stream_of[f] : 0]++] = f;
    for (int s = streams; s > 0; --s) starts[s] = starts[s - 1];
    starts[0] = 0;
    return 0;
}

}  // namespace fh
