// gallery_tags.hip — watchlists: every row carries a 32-bit TAG (a bit set of caller-defined groups), every query a 32-bit MASK, and
// row r is admitted for query q iff (tag[r] & mask[q]) != 0.  A tagged query is answered with the exact top-k of its admitted rows:
//   * the scan is the same code (gallery_scan.h) instantiated with TAGS — the predicate sits inside the push test, so the per-query
//     threshold is the k-th ADMITTED row and an excluded row can neither be listed nor push an admitted one out;
//   * scores, order (score desc, global row index asc), empty slots and the identity rule (an identity is represented by its best
//     ADMITTED row) are those of the untagged scans; the two-pass launcher and the merge kernels are reused as they are;
//   * tile_or[t] = the OR of the tags of rows [128 t, 128 t + 128): a workgroup whose 64 masks share no bit with it skips the tile
//     without loading it, so a selective query against grouped enrolments reads a fraction of the gallery.
// Here too: the kernel that keeps tile_or in step with the tags, the tag OR of template pooling (one thread per identity over the
// inverted index fuse builds) and the per-query masks of the tracker's identify call (one mask per stream).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "gallery_scan.h"
#include "kernels.h"

namespace fh {

__global__ __launch_bounds__(256, 2) void gallery_topk_tagged_kernel(const GalArgs p) { gallery_scan_body<float, GAL_KMAX, false, false, true>(p); }
__global__ __launch_bounds__(256, 2) void gallery_topk_ids_tagged_kernel(const GalArgs p) { gallery_scan_body<float, GAL_KMAX, false, true, true>(p); }

static_assert(GAL_TAG_TILE == GAL_BM, "tile_or is kept per row tile of the scan");

// one wave per row tile: tile_or[t] = OR of tags[128 t .. 128 t + 128) (rows behind G count as 0)
__global__ __launch_bounds__(64) void tag_tile_or_kernel(const unsigned* __restrict__ tags, long G, long tile0, unsigned* __restrict__ tile_or) {
    const long t = tile0 + blockIdx.x, r = t * GAL_BM + threadIdx.x;
    unsigned m = (r < G ? tags[r] : 0u) | (r + 64 < G ? tags[r + 64] : 0u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m |= (unsigned)__shfl_xor((int)m, o);
    if (threadIdx.x == 0) tile_or[t] = m;
}
// rebuilds the entries of the tiles that rows [first, first + n) touch
void launch_tag_tile_or(const unsigned* tags, long G, long first, long n, unsigned* tile_or, hipStream_t s) {
    if (n <= 0 || G <= 0) return;
    const long t0 = first / GAL_BM, t1 = (std::min(first + n, G) - 1) / GAL_BM;
    if (t1 < t0) return;
    hipLaunchKernelGGL(tag_tile_or_kernel, dim3((unsigned)(t1 - t0 + 1)), dim3(64), 0, s, tags, G, t0, tile_or);
}

// template pooling: dst row j = identity j = src rows order[starts[j] .. starts[j + 1])
__global__ __launch_bounds__(256) void fuse_tags_kernel(const unsigned* __restrict__ src_tags, const int* __restrict__ order,
                                                        const long long* __restrict__ starts, long m, unsigned* __restrict__ dst_tags) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    unsigned t = 0;
    for (long long i = starts[j]; i < starts[j + 1]; ++i) t |= src_tags[order[i]];
    dst_tags[j] = t;
}
void launch_fuse_tags(const unsigned* src_tags, const int* order, const long long* starts, long m, unsigned* dst_tags, hipStream_t s) {
    if (m <= 0) return;
    hipLaunchKernelGGL(fuse_tags_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, src_tags, order, starts, m, dst_tags);
}

// the tracker's watchlist per camera: position i of the stream plan is frame order[i] of the stream that owns i, and that frame's
// queries are [frame_off[f], frame_off[f + 1]) — each gets its stream's mask
__global__ __launch_bounds__(256) void track_query_masks_kernel(const unsigned* __restrict__ stream_mask, int streams, const int* __restrict__ order,
                                                                const int* __restrict__ starts, const int* __restrict__ frame_off, int n,
                                                                int total, unsigned* __restrict__ qmask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = streams;                                 // the stream s with starts[s] <= i < starts[s + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= i) lo = mid; else hi = mid;
    }
    const unsigned m = stream_mask[lo];
    const int f = order[i];
    const int j1 = min(frame_off[f + 1], total);              // (qmask holds `total` words)
    for (int j = max(frame_off[f], 0); j < j1; ++j) qmask[j] = m;
}
void launch_track_query_masks(const unsigned* stream_mask, int streams, const TrackCall& c, unsigned* qmask, hipStream_t s) {
    if (c.n <= 0) return;
    hipLaunchKernelGGL(track_query_masks_kernel, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, s, stream_mask, streams, c.order, c.starts,
                       c.frame_off, c.n, c.total, qmask);
}

}  // namespace fh
