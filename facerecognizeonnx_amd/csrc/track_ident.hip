// track_ident.hip — per-track identity on the device (contract: include/facehip.h, "track identity"; fh_track_identify_dev).  After an
// update the flagged faces of a call have embeddings; stage A pools each of them into its track's running template and writes one query
// row per flagged face, the gallery labels all queries at once (the existing 1:N calls, no code here), and stage C carries the answers
// to every face of the call.  Both kernels walk a stream's entries in the order of track_plan.h, 64 entries per round.
//   * the SUMS are plain fp32 additions in time order, so they reproduce bit for bit (tests/track_ident_model.py restates them); the
//     unit form is FaceRecognizer::normalize (src/face_recognizer.cpp:306-318) with gallery_fuse.hip's reduction: a lane-strided sum
//     of squares, then a butterfly.  Compiled with -ffp-contract=off, as track.hip.
//   * no atomics and nothing that depends on timing: a (stream, slot) chain belongs to one wave, a stream's labels to one wave.
//   * with track re-linking on (include/facehip.h, "track re-linking") stage A is track_link_kernel instead: one workgroup per stream.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "track_dev.h"

namespace fh {

// The flagged entries before each frame (track_select_kernel's prefix, kept): frame_off[0 .. n].  n <= 4096 frames.
__global__ __launch_bounds__(256) void track_ranks_kernel(const int* __restrict__ embed, int n, int per_frame, int* __restrict__ frame_off) {
    __shared__ int offs[4097];
    flagged_prefix(embed, n, per_frame, offs);
    for (int b = threadIdx.x; b <= n; b += 256) frame_off[b] = offs[b];
}

// ------------------------------------------------------------------------------------------
// Stage A.  Wave (s, l), l < max_tracks, owns slot l of stream s: it picks the flagged entries whose slot is l with a ballot and runs
// their chain in time order, every face through pool_row (track_dev.h) — (re)open: sum = row, query = row verbatim; else sum += row
// (POOL_SUM; POOL_LAST: sum = row, query = row) and the query is the normalised sum.  POOL_WEIGHTED is POOL_SUM with every row entering
// the sum as wq * row, wq = (float)max(quality, 1): one multiply, then one add per component (the file is built without contraction).
// Wave (s, max_tracks) copies the rows of the stream's untracked faces.  Each lane owns the 16-byte columns lane, lane + 64, ...; the
// sum row lives in the state and is read, added to and written back by the lane that owns the column.
// A flagged entry of rank >= total is nobody's.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void track_pool_kernel(TrackIdent* __restrict__ ident, float4* __restrict__ sums, int streams,
                                                         int max_tracks, int vpr, int pool, const int* __restrict__ track,
                                                         const int* __restrict__ slot, const int* __restrict__ embed,
                                                         const int* __restrict__ quality, const int* __restrict__ frame_off, const float4* __restrict__ emb, int total,
                                                         int per_frame, const int* __restrict__ order, const int* __restrict__ starts,
                                                         float4* __restrict__ queries) {
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (w >= streams * (max_tracks + 1)) return;
    const int s = w / (max_tracks + 1), l = w - s * (max_tracks + 1);
    const int my = l < max_tracks ? l : -1;                              // -1: the untracked faces
    const int b = starts[s], e = starts[s + 1];
    if (b == e) return;
    TrackIdent* const id = ident + (size_t)s * max_tracks + (my < 0 ? 0 : my);
    float4* const sm = sums + ((size_t)s * max_tracks + (my < 0 ? 0 : my)) * vpr;
    int owner = -1, n_emb = 0;
    if (my >= 0) { owner = id->owner; n_emb = id->n_emb; }
    const bool weighted = pool == kTrackPoolWeighted;

    walk_entries(order, b, e, per_frame, embed, frame_off, lane, [&](bool, int, int, size_t idx, bool fl, int rank) {
        const int sl = fl ? slot[idx] : -2;
        const int tid = fl ? track[idx] : -1;
        const int qual = (weighted && fl) ? quality[idx] : 1;
        unsigned long long m = __ballot(fl && rank < total && sl == my);
        while (m != 0) {                                                 // ascending lanes = (frame, slot) order = time order
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int q_e = __shfl(rank, src), t_e = __shfl(tid, src);
            const float wq = (float)max(__shfl(qual, src), 1);
            const float4* const row = emb + (size_t)q_e * vpr;
            float4* const q = queries + (size_t)q_e * vpr;
            if (my < 0) {
                for (int c = lane; c < vpr; c += 64) q[c] = row[c];
            } else {
                const bool open = owner != t_e;
                if (open) { owner = t_e; n_emb = 1; } else ++n_emb;
                pool_row(sm, sm, row, q, nullptr, wq, weighted, !open && pool != kTrackPoolLast, lane, vpr);
            }
        }
    });
    if (my >= 0 && lane == 0) { id->owner = owner; id->n_emb = n_emb; }
}

// ------------------------------------------------------------------------------------------
// Stage C.  One wave per stream; lane l holds (owner, label, score) of slot l in registers for the whole walk (loaded once, stored
// once), as track_update_kernel holds its slots.  A round's frames are taken in time order; inside one frame a slot occurs at most
// once, so its carried reads (a shuffle from the slot's lane) and its refreshes (one step per flagged face) do not meet.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void track_propagate_kernel(TrackIdent* __restrict__ ident, int max_tracks, const int* __restrict__ track,
                                                             const int* __restrict__ slot, const int* __restrict__ embed,
                                                             const int* __restrict__ frame_off, const int* __restrict__ ans_label,
                                                             const float* __restrict__ ans_score, int total, int per_frame,
                                                             const int* __restrict__ order, const int* __restrict__ starts,
                                                             int* __restrict__ label, float* __restrict__ score) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int b = starts[s], e = starts[s + 1];
    if (b == e) return;
    const bool usable = lane < max_tracks;
    TrackIdent st = kFreeIdent;
    if (usable) st = ident[(size_t)s * max_tracks + lane];

    walk_entries(order, b, e, per_frame, embed, frame_off, lane, [&](bool valid, int k, int nk, size_t idx, bool fl, int rank) {
        const int sl = valid ? slot[idx] : -1;
        const int tid = valid ? track[idx] : -1;
        int ol = -1;
        float os = -1.0f;
        const bool known = fl && rank < total;                           // a flagged entry behind `total` answers (-1, -1) and changes nothing
        if (known) { ol = ans_label[rank]; os = ans_score[rank]; }
        const bool upd = known && sl >= 0, carry = valid && !fl && sl >= 0;
        for (int kk = 0; kk < nk; ++kk) {
            if (__ballot(carry && k == kk) != 0) {
                const int cl = __shfl(st.label, sl & 63);
                const float cs = __shfl(st.score, sl & 63);
                if (carry && k == kk) { ol = cl; os = cs; }
            }
            unsigned long long m = __ballot(upd && k == kk);
            while (m != 0) {
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int t_slot = __shfl(sl, src), t_id = __shfl(tid, src), t_label = __shfl(ol, src);
                const float t_score = __shfl(os, src);
                if (lane == t_slot) { st.owner = t_id; st.label = t_label; st.score = t_score; }
            }
        }
        if (valid) { label[idx] = ol; score[idx] = os; }
    });
    if (usable) {
        TrackIdent* const id = ident + (size_t)s * max_tracks + lane;
        id->owner = st.owner; id->label = st.label; id->score = st.score;      // (n_emb is stage A's)
    }
}

// ------------------------------------------------------------------------------------------
// Stage A with re-linking on (include/facehip.h, "track re-linking").  A newly opened track may continue a LOST one, whose template sits
// in another row of the stream's table, so a stream's chains are no longer independent: ONE workgroup of four waves walks the stream's
// entries serially, in walk_entries's order (every wave walks; the walk and the slots' owners — lane l of EVERY wave holds slot l's —
// are replicated, so all four agree on where the open events are without talking).
//   * wave 0 owns the table (a copy in LDS, loaded once, stored once) and the sums: it is the only writer of both, and every one of its
//     lanes performs the same record updates, so each lane reads back what it wrote itself;
//   * wave 1 copies the untracked faces' rows, which touch no state;
//   * at an OPEN event the four waves meet (barrier: wave 0's table and sums become visible), wave w scores rows w, w + 4, ... — lanes
//     over the 16-byte columns, dot and sum of squares in the order the contract states — and keeps its best (score, owner); the four
//     bests meet in LDS (barrier) and wave 0 folds them in wave order, moves the records and pools the face.
// No atomics, nothing that depends on timing: every barrier is reached by all four waves under conditions that all four evaluate alike.
// ------------------------------------------------------------------------------------------
namespace {
// a candidate (score, owner, row); row < 0 = none
__device__ __forceinline__ void link_put(TrackLink& d, int owner, int root, int n_emb, int label, float score, int last_seen, int links) {
    d.owner = owner; d.root = root; d.n_emb = n_emb; d.label = label; d.score = score; d.last_seen = last_seen; d.links = links; d.pad = 0;
}
// (a) beats (b): the higher score, then the smaller owner; row < 0 = nothing yet
__device__ __forceinline__ bool link_beats(float a_score, int a_owner, int a_row, float b_score, int b_owner, int b_row) {
    return a_row >= 0 && (b_row < 0 || a_score > b_score || (a_score == b_score && a_owner < b_owner));
}
}  // namespace

__global__ __launch_bounds__(256) void track_link_kernel(TrackLink* __restrict__ links, TrackIdent* __restrict__ ident,
                                                         float4* __restrict__ sums, float4* __restrict__ msums,
                                                         const int* __restrict__ heads, int max_tracks, TrackLinkParams lp, int vpr, int pool,
                                                         const int* __restrict__ track, const int* __restrict__ slot,
                                                         const int* __restrict__ embed, const int* __restrict__ quality,
                                                         const int* __restrict__ frame_off, const float4* __restrict__ emb, int total,
                                                         int per_frame, const int* __restrict__ order, const int* __restrict__ starts,
                                                         float4* __restrict__ queries, int* __restrict__ root) {
    __shared__ TrackLink tab[64 + kTrackLinkMemory];
    __shared__ float best_score[4];
    __shared__ int best_owner[4], best_row[4];
    const int s = blockIdx.x, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = starts[s], e = starts[s + 1];
    if (b == e) return;
    const int R = max_tracks + lp.memory;
    TrackLink* const mine_rows = links + (size_t)s * R;
    for (int r = threadIdx.x; r < R; r += 256) {
        tab[r] = mine_rows[r];
        if (r < max_tracks) {                                            // a slot's (label, score) are stage C's: what the last call left
            const TrackIdent* const id = ident + (size_t)s * max_tracks + r;
            tab[r].label = id->label; tab[r].score = id->score;
        }
    }
    __syncthreads();
    const int frame_no = heads[2 * s];
    int owner = lane < max_tracks ? tab[lane].owner : -1;
    const bool weighted = pool == kTrackPoolWeighted;
    const int pieces = per_frame <= 64 ? 1 : (per_frame + 63) / 64;     // body calls per frame (per_frame > 64: one frame in pieces)
    int pos = b, piece = 0;
    float4* const slot_sums = sums + (size_t)s * max_tracks * vpr;
    float4* const mem_sums = msums + (size_t)s * lp.memory * vpr;
    auto sum_row = [&](int r) { return r < max_tracks ? slot_sums + (size_t)r * vpr : mem_sums + (size_t)(r - max_tracks) * vpr; };

    walk_entries(order, b, e, per_frame, embed, frame_off, lane, [&](bool valid, int k, int nk, size_t idx, bool fl, int rank) {
        const int sl = valid ? slot[idx] : -1;
        const int tid = valid ? track[idx] : -1;
        const bool known = fl && rank < total;
        const int qual = (weighted && known) ? quality[idx] : 1;
        int root_out = -1;
        for (int kk = 0; kk < nk; ++kk) {
            const int t = frame_no - (e - (pos + kk));                   // the update's frame time of this frame
            const bool here = valid && k == kk;
            unsigned long long un = __ballot(here && known && sl < 0);
            if (wave == 1) {
                while (un != 0) {
                    const int src = __ffsll((long long)un) - 1;
                    un &= un - 1;
                    const int q_e = __shfl(rank, src);
                    const float4* const row = emb + (size_t)q_e * vpr;
                    float4* const q = queries + (size_t)q_e * vpr;
                    for (int c = lane; c < vpr; c += 64) q[c] = row[c];
                }
            }
            const bool tracked = sl >= 0 && sl < max_tracks;             // (a slot the update cannot have written is nobody's)
            unsigned long long ev = __ballot(here && known && tracked);
            unsigned long long rest = __ballot(here && !known && tracked);
            // steps 3 and 4 of the entries that pool nothing, lane-parallel (a frame holds a slot at most once), kept in the serial
            // order relative to the events: the ones below an event's lane are done before it
            auto passive = [&](unsigned long long m) {
                if (wave == 0 && ((m >> lane) & 1ull) != 0 && tab[sl].owner == tid) {
                    tab[sl].last_seen = t;
                    root_out = tab[sl].root;
                }
                __builtin_amdgcn_wave_barrier();
            };
            while (ev != 0) {
                const int src = __ffsll((long long)ev) - 1;
                ev &= ev - 1;
                const unsigned long long below = (1ull << src) - 1ull;
                if ((rest & below) != 0) { passive(rest & below); rest &= ~below; }
                const int q_e = __shfl(rank, src), t_e = __shfl(tid, src), s_e = __shfl(sl, src);
                const float wq = (float)max(__shfl(qual, src), 1);
                const float4* const row = emb + (size_t)q_e * vpr;
                float4* const q = queries + (size_t)q_e * vpr;
                float4* const sm = slot_sums + (size_t)s_e * vpr;
                const bool open = __shfl(owner, s_e) != t_e;
                if (!open) {                                             // 2. a continued track
                    if (wave == 0) {
                        tab[s_e].n_emb += 1;
                        tab[s_e].last_seen = t;
                        if (lane == src) root_out = tab[s_e].root;
                        pool_row(sm, sm, row, q, nullptr, wq, weighted, pool != kTrackPoolLast, lane, vpr);
                    }
                    continue;
                }
                // 1. an open event
                __syncthreads();                                         // wave 0's table and sums, as they stand now
                float m_score = 0.f;
                int m_owner = 0, m_row = -1;
                for (int r = wave; r < R; r += 4) {
                    const int c_owner = tab[r].owner, gap = t - tab[r].last_seen - 1;
                    if (c_owner == -1 || gap <= lp.max_missed || gap > lp.max_age) continue;      // not dead at t, or out of reach
                    const float4* const cs = sum_row(r);
                    float d = 0.f, ss = 0.f;
                    for (int c = lane; c < vpr; c += 64) {
                        const float4 a = cs[c], v = row[c];
                        d += v.x * a.x + v.y * a.y + v.z * a.z + v.w * a.w;
                        ss += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
                    }
                    d = wave_sum(d);
                    ss = wave_sum(ss);
                    const float nrm = sqrtf(ss);
                    const float cosv = nrm > 0.f ? d / nrm : d;
                    const float c_score = (cosv + 1.0f) * 0.5f;
                    if (c_score > lp.link_thr && link_beats(c_score, c_owner, r, m_score, m_owner, m_row)) {      // (a NaN never exceeds it)
                        m_score = c_score; m_owner = c_owner; m_row = r;
                    }
                }
                if (lane == 0) { best_score[wave] = m_score; best_owner[wave] = m_owner; best_row[wave] = m_row; }
                __syncthreads();
                float w_score = best_score[0];
                int w_owner = best_owner[0], w_row = best_row[0];
                for (int w = 1; w < 4; ++w)
                    if (link_beats(best_score[w], best_owner[w], best_row[w], w_score, w_owner, w_row)) {
                        w_score = best_score[w]; w_owner = best_owner[w]; w_row = best_row[w];
                    }
                if (lane == w_row) owner = -1;                         // every wave: a slot row that is taken is free ...
                if (lane == s_e) owner = t_e;                            // ... and the slot is this track's now, linked or not
                if (wave != 0) continue;
                // (the records travel as scalars: whole-struct copies chosen at run time would live in scratch)
                const int o_owner = tab[s_e].owner, o_root = tab[s_e].root, o_n = tab[s_e].n_emb, o_label = tab[s_e].label;
                const float o_score = tab[s_e].score;
                const int o_seen = tab[s_e].last_seen, o_links = tab[s_e].links;
                const int old_gap = t - o_seen - 1;
                bool retire = o_owner != -1 && old_gap > lp.max_missed && old_gap <= lp.max_age && lp.memory > 0;
                int r_root = t_e, r_n = 1, r_label = -1, r_links = 0;    // no winner: the slot opens as today, unnamed
                float r_score = -1.0f;
                if (w_row >= 0) {                                      // the winner's record, continued
                    const TrackLink& c = tab[w_row];
                    r_root = c.root; r_n = c.n_emb + 1; r_label = c.label; r_score = c.score; r_links = c.links + 1;
                    link_put(tab[w_row], -1, -1, 0, -1, -1.0f, 0, 0);
                    if (w_row == s_e) retire = false;
                }
                int to = -1;                                             // the memory row the old record retires to
                if (retire) {
                    for (int m0 = 0; m0 < lp.memory && to < 0; m0 += 64) {
                        const int m = m0 + lane;
                        bool avail = false;
                        if (m < lp.memory) {
                            const TrackLink& x = tab[max_tracks + m];
                            avail = x.owner == -1 || t - x.last_seen - 1 > lp.max_age;
                        }
                        const unsigned long long am = __ballot(avail);
                        if (am != 0) to = max_tracks + m0 + __ffsll((long long)am) - 1;
                    }
                    if (to < 0) {                                        // all in reach: the smallest last_seen goes, then the smaller owner
                        int b_seen = 0x7fffffff, b_owner = 0x7fffffff, b_row = -1;
                        for (int m = lane; m < lp.memory; m += 64) {
                            const TrackLink& x = tab[max_tracks + m];
                            if (b_row < 0 || x.last_seen < b_seen || (x.last_seen == b_seen && x.owner < b_owner)) {
                                b_seen = x.last_seen; b_owner = x.owner; b_row = max_tracks + m;
                            }
                        }
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) {
                            const int o_seen = __shfl_xor(b_seen, o), o_owner = __shfl_xor(b_owner, o), o_row = __shfl_xor(b_row, o);
                            if (o_row >= 0 && (b_row < 0 || o_seen < b_seen || (o_seen == b_seen && o_owner < b_owner))) {
                                b_seen = o_seen; b_owner = o_owner; b_row = o_row;
                            }
                        }
                        to = b_row;
                    }
                }
                // the sums: the old ones retire to row `to`, the face joins the winner's (a resumed POOL_LAST track and a new one: sum =
                // the face).  pool_row reads every column whole before it writes it, so the three rows may coincide
                pool_row(sm, w_row >= 0 ? sum_row(w_row) : sm, row, q, to >= 0 ? sum_row(to) : nullptr, wq, weighted,
                         w_row >= 0 && pool != kTrackPoolLast, lane, vpr);
                if (to >= 0) link_put(tab[to], o_owner, o_root, o_n, o_label, o_score, o_seen, o_links);
                link_put(tab[s_e], t_e, r_root, r_n, r_label, r_score, t, r_links);
                if (lane == src) root_out = r_root;
            }
            if (rest != 0) passive(rest);
        }
        if (wave == 0 && valid) root[idx] = root_out;
        if (++piece == pieces) { piece = 0; pos += nk; }
    });
    __syncthreads();
    for (int r = threadIdx.x; r < R; r += 256) {
        mine_rows[r] = tab[r];
        if (r < max_tracks) {
            TrackIdent* const id = ident + (size_t)s * max_tracks + r;
            id->owner = tab[r].owner; id->n_emb = tab[r].n_emb;          // (label and score are stage C's)
        }
    }
}

__global__ __launch_bounds__(256) void track_roots_kernel(const int* __restrict__ track, const int* __restrict__ slot, long entries,
                                                          int* __restrict__ root) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < entries) root[i] = slot[i] >= 0 ? track[i] : -1;
}

// The launchers unpack the call into the kernels' own parameters: a pointer that arrives inside a struct loses its __restrict__.
void launch_track_link(const TrackIdentState& st, TrackLink* links, float* msums, const int* heads, TrackLinkParams lp, const TrackCall& c,
                       const float* emb, float* queries, int* root, hipStream_t s) {
    hipLaunchKernelGGL(track_link_kernel, dim3(st.streams), dim3(256), 0, s, links, st.ident, reinterpret_cast<float4*>(st.sums),
                       reinterpret_cast<float4*>(msums), heads, st.max_tracks, lp, st.dim / 4, st.pool, c.track, c.slot, c.embed, c.quality,
                       c.frame_off, reinterpret_cast<const float4*>(emb), c.total, c.per_frame, c.order, c.starts,
                       reinterpret_cast<float4*>(queries), root);
}

void launch_track_roots(const int* track, const int* slot, long entries, int* root, hipStream_t s) {
    hipLaunchKernelGGL(track_roots_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, track, slot, entries, root);
}

void launch_track_ranks(const TrackCall& c, hipStream_t s) {
    hipLaunchKernelGGL(track_ranks_kernel, dim3(1), dim3(256), 0, s, c.embed, c.n, c.per_frame, c.frame_off);
}

void launch_track_pool(const TrackIdentState& st, const TrackCall& c, const float* emb, float* queries, hipStream_t s) {
    const int waves = st.streams * (st.max_tracks + 1);
    hipLaunchKernelGGL(track_pool_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, st.ident, reinterpret_cast<float4*>(st.sums),
                       st.streams, st.max_tracks, st.dim / 4, st.pool, c.track, c.slot, c.embed, c.quality, c.frame_off,
                       reinterpret_cast<const float4*>(emb), c.total, c.per_frame, c.order, c.starts, reinterpret_cast<float4*>(queries));
}

void launch_track_propagate(const TrackIdentState& st, const TrackCall& c, const int* ans_label, const float* ans_score, int* label,
                            float* score, hipStream_t s) {
    hipLaunchKernelGGL(track_propagate_kernel, dim3(st.streams), dim3(64), 0, s, st.ident, st.max_tracks, c.track, c.slot, c.embed,
                       c.frame_off, ans_label, ans_score, c.total, c.per_frame, c.order, c.starts, label, score);
}

}  // namespace fh
