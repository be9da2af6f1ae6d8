// gallery_ids.hip — the LABELLED gallery: every enrolled row carries an identity id, and a query is answered with its best k
// identities instead of its best k rows (a person enrolled with 20 templates takes one slot, not sixteen).
//   * row score: exactly gallery_topk_kernel's — the scan is the same code (gallery_scan.h), instantiated with identity-aware lists;
//   * order: entry (s, r) is better than (s', r') iff s > s', or s == s' and r < r' (r = global row index);
//   * an identity's representative is its best row; the answer is the first k representatives; a slot holds (score, id, row), an
//     empty slot (-1.0f, -1, -1); NaN scores are never listed.
// Per-workgroup lists go to memory as [part][Q][k] in three planes; topk_merge_kernel<CACHED, true> (gallery.hip) selects the
// overall answer.  It is also the merge step of a row-sharded labelled gallery (fh_topk_merge_ids_dev), because per-part identity lists suffice:
//   suppose identity X is in the global answer and its representative lies in part p.  Every identity ahead of X within part p has a
//   part-best at least as good as X's representative, so its global best is at least as good, and it is ahead of X globally as well.
//   Fewer than k identities are ahead of X globally, so fewer than k are ahead of X in part p: X is in part p's list, with that same
//   representative.  De-duplicating the union of the part lists (keep an identity's best entry) therefore yields the global answer.
// The same argument keeps the seed pass valid: if k distinct identities of a prefix score at least tau, tau admits every member of
// the final answer.  What changes against the row-level scan is the overflow replay: many templates of one identity can pass the
// threshold of a tile while the list does not tighten (they share one slot), so the four-round replay fires more often.
// Removal (fh_gallery_remove_ids) is a stable compaction: a host-built list of the surviving positions, then a gather of whole rows
// (fp32 rows, ids, fp16 rows) into a second buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <stdexcept>

#include "gallery_scan.h"
#include "kernels.h"

namespace fh {

__global__ __launch_bounds__(256, 2) void gallery_topk_ids_kernel(const GalArgs p) { gallery_scan_body<float, GAL_KMAX, false, true>(p); }

__global__ void ids_of_rows_kernel(const float* __restrict__ score, const int* __restrict__ idx, int n, const int* __restrict__ ids, long idx_base,
                                   float thr, int use_thr, int* __restrict__ out_id) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = idx[i];
    out_id[i] = (r >= 0 && (!use_thr || score[i] > thr)) ? ids[(long)r - idx_base] : -1;
}
void launch_ids_of_rows(const float* score, const int* idx, int n, const int* ids, long idx_base, float thr, bool use_thr, int* out_id,
                        hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(ids_of_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, s, score, idx, n, ids, idx_base, thr, use_thr ? 1 : 0, out_id);
}

// dst row j = src row map[j], 16 bytes per thread
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const int* __restrict__ map,
                                                          long m, int vec_per_row) {
    const long total = m * vec_per_row;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long j = e / vec_per_row;
        const int c = (int)(e - j * vec_per_row);
        dst[e] = src[(long)map[j] * vec_per_row + c];
    }
}
void launch_gather_rows(const void* src, void* dst, const int* map, long m, size_t row_bytes, hipStream_t s) {
    if (m <= 0) return;
    if (row_bytes % 16) throw std::runtime_error("gallery: row size must be a multiple of 16 bytes");
    const int vpr = (int)(row_bytes / 16);
    const long blocks = std::min<long>((m * vpr + 255) / 256, 65536);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint4*>(src), static_cast<uint4*>(dst), map, m, vpr);
}
__global__ void gather_ids_kernel(const int* __restrict__ src, int* __restrict__ dst, const int* __restrict__ map, long m) {
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (long)gridDim.x * blockDim.x) dst[j] = src[map[j]];
}
void launch_gather_ids(const int* src, int* dst, const int* map, long m, hipStream_t s) {
    if (m <= 0) return;
    const long blocks = std::min<long>((m + 255) / 256, 65536);
    hipLaunchKernelGGL(gather_ids_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, map, m);
}

}  // namespace fh
