// tracker.cpp — the host side of fh::Tracker (engine.h): the per-stream state on the device, its clears and read-backs, and the launch
// sequences of the update (track.hip) and of the identify step (track_ident.hip, the gallery's label call, gallery_tags.hip).
#include "engine.h"
#include "track_plan.h"

#include <algorithm>

namespace fh {

namespace {
// `count` elements at src (device) as a host vector
template <class T>
std::vector<T> fetch(const T* src, size_t count) {
    std::vector<T> v(count);
    FH_HIP(hipMemcpy(v.data(), src, count * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}
// of(i) for the live slots i of `all`, ascending, into out[0 .. live), the rest of out[all.size()] = free_rec; out may be null (of is
// still called).  Returns live.
template <class T, class Of>
int compact_live(const std::vector<TrackState>& all, T* out, const T& free_rec, Of&& of) {
    int live = 0;
    for (size_t i = 0; i < all.size(); ++i) {
        if (all[i].id < 0) continue;
        const T v = of(i);
        if (out) out[live] = v;
        ++live;
    }
    if (out) std::fill(out + live, out + all.size(), free_rec);
    return live;
}
}  // namespace

Tracker::Tracker(int streams, int max_tracks, float iou_thr, int max_missed, int refresh)
    : streams_(streams), p_{max_tracks, iou_thr, max_missed, refresh, 1, 1, 1} {
    state_.ensure((size_t)streams * (2 * sizeof(int) + (size_t)max_tracks * sizeof(TrackState)));
    reset(-1);
}

void Tracker::reset(int stream) {
    FH_HIP(hipDeviceSynchronize());                              // a queued update still reads and writes the state
    const int first = stream < 0 ? 0 : stream, count = stream < 0 ? streams_ : 1;
    FH_HIP(hipMemset(heads() + 2 * (size_t)first, 0, (size_t)count * 2 * sizeof(int)));
    const std::vector<TrackState> free_slots((size_t)count * p_.max_tracks, kFreeTrack);
    FH_HIP(hipMemcpy(slots() + (size_t)first * p_.max_tracks, free_slots.data(), free_slots.size() * sizeof(TrackState), hipMemcpyHostToDevice));
    if (idim_ > 0) clear_identity(first, count);                 // track ids restart at 0: a stale owner must not survive
    if (relink_) clear_links(first, count);
    if (best_.p) FH_HIP(hipMemset(best_.as<int>() + (size_t)first * p_.max_tracks, 0, (size_t)count * p_.max_tracks * sizeof(int)));
}

void Tracker::set_bestshot(bool on, int num, int den, int min_gap) {
    FH_HIP(hipDeviceSynchronize());                              // a queued update still reads and writes best_q
    const size_t bytes = (size_t)streams_ * p_.max_tracks * sizeof(int);
    best_.ensure(bytes);
    FH_HIP(hipMemset(best_.p, 0, bytes));
    bestshot_ = on;
    p_.bs_num = num; p_.bs_den = den; p_.bs_gap = min_gap;
}

void Tracker::clear_identity(int first, int count) {
    const size_t entries = (size_t)count * p_.max_tracks, at = (size_t)first * p_.max_tracks;
    const std::vector<TrackIdent> none(entries, kFreeIdent);
    FH_HIP(hipMemcpy(ident_.as<TrackIdent>() + at, none.data(), entries * sizeof(TrackIdent), hipMemcpyHostToDevice));
    FH_HIP(hipMemset(isum_.as<float>() + at * idim_, 0, entries * idim_ * sizeof(float)));
}

void Tracker::enable_identity(int dim, int pool) {
    FH_HIP(hipDeviceSynchronize());                              // a queued identify still reads and writes the state
    const size_t entries = (size_t)streams_ * p_.max_tracks;
    ident_.ensure(entries * sizeof(TrackIdent));
    isum_.ensure(entries * dim * sizeof(float));
    idim_ = dim; ipool_ = pool;
    relink_ = false;
    clear_identity(0, streams_);
}

void Tracker::set_stream_masks(const unsigned* masks_host) {
    FH_HIP(hipDeviceSynchronize());                              // a queued identify still reads the masks
    masks_on_ = masks_host != nullptr;
    if (!masks_on_) return;
    smask_.ensure((size_t)streams_ * sizeof(unsigned));
    FH_HIP(hipMemcpy(smask_.p, masks_host, (size_t)streams_ * sizeof(unsigned), hipMemcpyHostToDevice));
}

void Tracker::clear_links(int first, int count) {
    const size_t rows = (size_t)link_rows(), entries = (size_t)count * rows;
    const std::vector<TrackLink> none(entries, kFreeLink);
    FH_HIP(hipMemcpy(link_.as<TrackLink>() + (size_t)first * rows, none.data(), entries * sizeof(TrackLink), hipMemcpyHostToDevice));
    const size_t per = (size_t)lp_.memory * idim_;
    if (per > 0) FH_HIP(hipMemset(msum_.as<float>() + (size_t)first * per, 0, (size_t)count * per * sizeof(float)));
}

void Tracker::enable_relink(int memory, float thr, int max_age) {
    FH_HIP(hipDeviceSynchronize());                              // a queued identify still reads and writes the state
    lp_ = TrackLinkParams{memory, thr, p_.max_missed, max_age};
    link_.ensure((size_t)streams_ * link_rows() * sizeof(TrackLink));
    msum_.ensure(std::max<size_t>((size_t)streams_ * memory * idim_ * sizeof(float), 16));
    relink_ = true;
    clear_identity(0, streams_);
    clear_links(0, streams_);
}

std::vector<TrackState> Tracker::slots_of(int stream) {
    FH_HIP(hipDeviceSynchronize());
    return fetch(slots() + (size_t)stream * p_.max_tracks, (size_t)p_.max_tracks);
}

int Tracker::get_state(int stream, TrackState* out, int* frame_no, int* next_id) {
    const std::vector<TrackState> all = slots_of(stream);
    const std::vector<int> head = fetch(heads() + 2 * (size_t)stream, 2);
    if (frame_no) *frame_no = head[0];
    if (next_id) *next_id = head[1];
    return compact_live(all, out, kFreeTrack, [&](size_t i) { return all[i]; });
}

int Tracker::get_quality(int stream, int* out) {
    const std::vector<TrackState> all = slots_of(stream);
    const std::vector<int> best = fetch(best_.as<int>() + (size_t)stream * all.size(), all.size());
    return compact_live(all, out, 0, [&](size_t i) { return best[i]; });
}

int Tracker::get_identity(int stream, TrackIdent* out, float* sums_out) {
    const std::vector<TrackState> all = slots_of(stream);
    const size_t at = (size_t)stream * all.size();
    const std::vector<TrackIdent> ident = fetch(ident_.as<TrackIdent>() + at, all.size());
    float* dst = sums_out;                                       // the next live slot's row
    return compact_live(all, out, kFreeIdent, [&](size_t i) {
        const bool mine = ident[i].owner == all[i].id;           // else: identify was skipped for this track
        if (dst) {
            if (mine) FH_HIP(hipMemcpy(dst, isum_.as<float>() + (at + i) * idim_, (size_t)idim_ * sizeof(float), hipMemcpyDeviceToHost));
            else std::fill(dst, dst + idim_, 0.0f);
            dst += idim_;
        }
        return mine ? TrackIdent{all[i].id, ident[i].n_emb, ident[i].label, ident[i].score} : TrackIdent{all[i].id, 0, -1, -1.0f};
    });
}

void Tracker::get_links(int stream, TrackLink* out, float* sums_out) {
    FH_HIP(hipDeviceSynchronize());
    const size_t mt = (size_t)p_.max_tracks, rows = (size_t)link_rows();
    FH_HIP(hipMemcpy(out, link_.as<TrackLink>() + (size_t)stream * rows, rows * sizeof(TrackLink), hipMemcpyDeviceToHost));
    const std::vector<TrackIdent> ident = fetch(ident_.as<TrackIdent>() + (size_t)stream * mt, mt);
    for (size_t i = 0; i < mt; ++i) {                            // a slot's (label, score) are stage C's; a free row reports nothing
        if (out[i].owner != -1) { out[i].label = ident[i].label; out[i].score = ident[i].score; }
        else out[i] = kFreeLink;
    }
    if (!sums_out) return;
    FH_HIP(hipMemcpy(sums_out, isum_.as<float>() + (size_t)stream * mt * idim_, mt * idim_ * sizeof(float), hipMemcpyDeviceToHost));
    if (lp_.memory > 0)
        FH_HIP(hipMemcpy(sums_out + mt * idim_, msum_.as<float>() + (size_t)stream * lp_.memory * idim_,
                         (size_t)lp_.memory * idim_ * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < rows; ++i)                            // a free row reports a zero sum
        if (out[i].owner == -1) std::fill(sums_out + i * idim_, sums_out + (i + 1) * idim_, 0.0f);
}

// The stream plan of track_plan.h (order[n], then starts[streams + 1]) through one of the two staging tables; returns the device copy.
const int* Tracker::send_plan(StagedTable& table, const int* stream_of, int n, hipStream_t s) {
    const size_t bytes = ((size_t)n + streams_ + 1) * sizeof(int);
    int* order = static_cast<int*>(table.stage(bytes));
    if (track_plan(stream_of, n, streams_, order, order + n) != 0) throw std::runtime_error("tracker: bad stream_of");   // (checked by the caller)
    return static_cast<const int*>(table.send(bytes, s));
}

void Tracker::update_dev(const FaceRec* det, const int* counts, int n, int per_frame, const int* stream_of, int* track, int* embed,
                         int* slot, const int* quality, hipStream_t s) {
    const int* d_order = send_plan(plan_, stream_of, n, s);
    launch_track_update(heads(), slots(), streams_, p_, det, counts, per_frame, d_order, d_order + n, track, embed, slot,
                        bestshot_ ? quality : nullptr, bestshot_ ? best_.as<int>() : nullptr, s);
    FH_HIP(hipGetLastError());
}

// Pool first, label the whole batch of queries, propagate afterwards: the gallery scan wants every query of the call at once, and only
// the per-slot chains of stages A and C are serial.
void Tracker::identify_dev(Gallery& g, float thr, const int* track, const int* slot, const int* embed, const int* quality, const float* emb,
                           int total, int n, int per_frame, const int* stream_of, int* label, float* score, hipStream_t s, int* root) {
    const int* d_order = send_plan(iplan_, stream_of, n, s);
    const size_t rows = (size_t)std::max(total, 1);
    queries_.ensure(rows * idim_ * sizeof(float));
    ans_label_.ensure(rows * sizeof(int));
    ans_score_.ensure(rows * sizeof(float));
    frame_off_.ensure(((size_t)n + 1) * sizeof(int));
    const TrackCall c{track, slot, embed, quality, frame_off_.as<int>(), d_order, d_order + n, n, per_frame, total};
    const TrackIdentState st{ident_.as<TrackIdent>(), isum_.as<float>(), streams_, p_.max_tracks, idim_, ipool_};
    launch_track_ranks(c, s);
    if (relink_) {
        launch_track_link(st, link_.as<TrackLink>(), msum_.as<float>(), heads(), lp_, c, emb, queries_.as<float>(), root, s);
    } else {
        launch_track_pool(st, c, emb, queries_.as<float>(), s);
        if (root) launch_track_roots(track, slot, (long)n * per_frame, root, s);
    }
    FH_HIP(hipGetLastError());
    const bool ids = g.labelled() && g.size() > 0;               // labels are identity ids / row indices
    if (masks_on_ && total > 0) {                                // a watchlist per camera: every query carries its stream's mask
        qmask_.ensure(rows * sizeof(unsigned));
        launch_track_query_masks(smask_.as<unsigned>(), streams_, c, qmask_.as<unsigned>(), s);
        FH_HIP(hipGetLastError());
    }
    for (int c0 = 0; c0 < total; c0 += 256) {
        const int Q = std::min(256, total - c0);
        const float* q = queries_.as<float>() + (size_t)c0 * idim_;
        g.label_dev(q, masks_on_ ? qmask_.as<unsigned>() + c0 : nullptr, Q, thr, ids, ans_label_.as<int>() + c0, ans_score_.as<float>() + c0, s);
    }
    launch_track_propagate(st, c, ans_label_.as<int>(), ans_score_.as<float>(), label, score, s);
    FH_HIP(hipGetLastError());
}

}  // namespace fh
