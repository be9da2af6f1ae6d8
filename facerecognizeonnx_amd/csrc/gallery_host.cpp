// gallery_host.cpp — the host side of fh::Gallery (engine.h): the row store (one capacity, the per-row columns that share it), the
// maintenance calls written on its three operations (reserve, append, compact), the two queries over the one fp32 scan sequence
// (gallery_scan.h: launch_gallery_scan) and the F16_RERANK path (gallery_f16.hip), the threshold search (gallery_range.hip) and the deep top-k (gallery_deep.hip).
#include "engine.h"

#include "gallery_scan.h"
#include "group_ids.h"
#include "roc_plan.h"

#include <algorithm>
#include <climits>
#include <cstring>

namespace fh {

// ------------------------------------------------------------------------------------------ the row store
namespace {
size_t tile_or_bytes(long rows) { return (size_t)((rows + GAL_TAG_TILE - 1) / GAL_TAG_TILE) * sizeof(unsigned); }
}

void Gallery::set_live(Column& c, bool on) {
    c.live = on;
    if (!on) return;
    c.buf.ensure((size_t)cap_ * c.row_bytes);
    if (&c == &tags_) tile_or_.ensure(tile_or_bytes(cap_));
}

void Gallery::reserve(long cap) {
    if (cap <= cap_) return;
    for (Column* c : cols_)
        if (c->live) c->buf.grow((size_t)cap * c->row_bytes, (size_t)n_ * c->row_bytes);
    if (tags_.live) tile_or_.grow(tile_or_bytes(cap), tile_or_bytes(n_));
    cap_ = cap;
}

long Gallery::append(long n) {
    if (n_ + n > cap_) reserve(std::max(n_ + n, 2 * cap_));      // grow geometrically, keeping the enrolled rows
    return n_;
}

// Stable compaction through second buffers: whole rows are gathered by the list of surviving positions (gallery_ids.hip; the 4-byte
// columns by the ids' gather), then the buffers change places.  tile_or keeps its size (m < the old row count: it fits) and is the
// caller's to rebuild.
void Gallery::compact(const int* map, long m) {
    DevBuf fresh[kCols];
    for (int i = 0; i < kCols; ++i) {
        const Column& c = *cols_[i];
        if (!c.live) continue;
        fresh[i].ensure((size_t)m * c.row_bytes);
        if (c.row_bytes == sizeof(int)) launch_gather_ids(c.as<int>(), fresh[i].as<int>(), map, m, nullptr);
        else launch_gather_rows(c.buf.p, fresh[i].p, map, m, c.row_bytes, nullptr);
    }
    FH_HIP(hipGetLastError());
    FH_HIP(hipDeviceSynchronize());
    for (int i = 0; i < kCols; ++i)
        if (cols_[i]->live) cols_[i]->buf.swap(fresh[i]);
    n_ = cap_ = m;
}

void Gallery::upload(const float* rows, const int* ids, long n, bool device_src, long index_base) {
    if (dim_ % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    if (!ids && n_ > 0 && ids_.live) throw std::runtime_error("gallery: the gallery is labelled: upload rows with their ids (fh_gallery_upload_ids)");
    const hipMemcpyKind kind = device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    n_ = 0;                                                      // a new row set: nothing to keep, every row admitted everywhere until set_tags
    set_live(ids_, ids != nullptr);
    set_live(tags_, false);
    reserve(n);
    FH_HIP(hipMemcpy(rows_.buf.p, rows, (size_t)n * rows_.row_bytes, kind));
    if (ids) FH_HIP(hipMemcpy(ids_.buf.p, ids, (size_t)n * sizeof(int), kind));
    n_ = n; base_ = index_base; fused_ = false;
    if (rows16_.live) convert16(0, n);
}

void Gallery::convert16(long first, long n) {
    gstat_.ensure(4 * sizeof(unsigned));
    if (first == 0) FH_HIP(hipMemset(gstat_.p, 0, 4 * sizeof(unsigned)));      // a new row set: fresh bounds (enroll keeps the maxima)
    launch_gallery16_convert(rows_.as<float>() + (size_t)first * dim_, rows16_.as<uint16_t>() + (size_t)first * dim_, n, dim_,
                             gstat_.as<unsigned>(), nullptr);
    FH_HIP(hipGetLastError());
    unsigned h[4];
    FH_HIP(hipMemcpy(h, gstat_.p, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) memcpy(&gbound_[i], &h[i], sizeof(float));
    f16_bad_ = h[3] != 0;
}

void Gallery::set_scan(int mode) {
    if (mode != 0 && mode != 1) throw std::invalid_argument("gallery: unknown scan mode");
    if (mode == 0) {
        set_live(rows16_, false);
        DevBuf none;
        none.swap(rows16_.buf);                                  // FP32 frees the copy
        return;
    }
    if (!rows16_.live) {
        ctr_.ensure(2 * sizeof(unsigned long long));
        FH_HIP(hipMemset(ctr_.p, 0, 2 * sizeof(unsigned long long)));
        set_live(rows16_, true);
        if (n_ > 0) convert16(0, n_);
    }
}

void Gallery::scan_stats(long long* certified, long long* fallback) {
    unsigned long long h[2] = {0, 0};
    FH_HIP(hipDeviceSynchronize());
    if (ctr_.p) {
        FH_HIP(hipMemcpy(h, ctr_.p, sizeof(h), hipMemcpyDeviceToHost));
        FH_HIP(hipMemset(ctr_.p, 0, sizeof(h)));
    }
    if (certified) *certified = (long long)h[0];
    if (fallback) *fallback = (long long)h[1] + host_fallback_;
    host_fallback_ = 0;
}

long Gallery::enroll(const float* rows, const int* ids, long n, bool device_src) {
    if (dim_ % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    if (n_ > 0 && ids_.live != (ids != nullptr))
        throw std::runtime_error(ids_.live ? "gallery: the gallery is labelled: enrol rows with their ids (fh_gallery_enroll_ids)"
                                           : "gallery: the gallery is unlabelled: fh_gallery_enroll_ids needs an empty or labelled gallery");
    const hipMemcpyKind kind = device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (n_ == 0) set_live(ids_, ids != nullptr);                 // an empty gallery takes either kind
    const long at = append(n);
    FH_HIP(hipMemcpy(rows_.as<float>() + (size_t)at * dim_, rows, (size_t)n * rows_.row_bytes, kind));
    if (rows16_.live) convert16(at, n);
    if (ids) FH_HIP(hipMemcpy(ids_.as<int>() + at, ids, (size_t)n * sizeof(int), kind));
    fused_ = false;                                              // appended ids are neither distinct nor in order
    n_ += n;
    if (tags_.live) {                                            // the new rows are admitted everywhere
        FH_HIP(hipMemset(tags_.as<unsigned>() + at, 0xFF, (size_t)n * sizeof(unsigned)));
        rebuild_tile_or(at, n);                                  // (from the old last tile on)
    }
    return base_ + at;
}

// Tags.  tile_or is rebuilt by position for the tiles a change touches (set_tags: its range; enroll: from the old last tile on;
// remove_ids and fuse: all of them).
void Gallery::rebuild_tile_or(long first, long n) {
    launch_tag_tile_or(tags_.as<unsigned>(), n_, first, n, tile_or_.as<unsigned>(), nullptr);
    FH_HIP(hipGetLastError());
    FH_HIP(hipDeviceSynchronize());
}

void Gallery::need_tags() {
    if (!tag_ctr_.p) {
        tag_ctr_.ensure(2 * sizeof(unsigned long long));
        FH_HIP(hipMemset(tag_ctr_.p, 0, 2 * sizeof(unsigned long long)));
    }
    if (tags_.live) return;
    set_live(tags_, true);
    if (n_ > 0) {
        FH_HIP(hipDeviceSynchronize());                          // a queued tagged scan of an earlier row set may still read the buffers
        FH_HIP(hipMemset(tags_.buf.p, 0xFF, (size_t)n_ * sizeof(unsigned)));
        rebuild_tile_or(0, n_);
    }
}

void Gallery::set_tags(long first, long n, const unsigned* tags, bool device_src) {
    if (first < 0 || n < 0 || first + n > n_) throw std::invalid_argument("gallery: tag range outside the gallery");
    if (n == 0) return;
    FH_HIP(hipDeviceSynchronize());                              // queued scans still read the tags that are about to change
    need_tags();
    FH_HIP(hipMemcpy(tags_.as<unsigned>() + first, tags, (size_t)n * sizeof(unsigned), device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    rebuild_tile_or(first, n);
}

void Gallery::get_tags(long first, long n, unsigned* out_host) {
    if (first < 0 || n < 0 || first + n > n_) throw std::invalid_argument("gallery: tag range outside the gallery");
    if (n == 0) return;
    if (!tags_.live) { std::fill(out_host, out_host + n, 0xFFFFFFFFu); return; }
    FH_HIP(hipDeviceSynchronize());
    FH_HIP(hipMemcpy(out_host, tags_.as<unsigned>() + first, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost));
}

void Gallery::tag_stats(long long* scanned, long long* skipped) {
    unsigned long long h[2] = {0, 0};
    FH_HIP(hipDeviceSynchronize());
    if (tag_ctr_.p) {
        FH_HIP(hipMemcpy(h, tag_ctr_.p, sizeof(h), hipMemcpyDeviceToHost));
        FH_HIP(hipMemset(tag_ctr_.p, 0, sizeof(h)));
    }
    if (scanned) *scanned = (long long)h[0];
    if (skipped) *skipped = (long long)h[1];
}

void Gallery::need_labelled(const std::string& what) const {
    if (n_ > 0 && !ids_.live) throw std::runtime_error("gallery: " + what + " needs a labelled gallery (rows enrolled with ids)");
}

void Gallery::get_ids(long first, long n, int* out_host) {
    need_labelled("fh_gallery_get_ids");
    if (first < 0 || n < 0 || first + n > n_) throw std::invalid_argument("gallery: id range outside the gallery");
    if (n > 0) FH_HIP(hipMemcpy(out_host, ids_.as<int>() + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
}

void Gallery::get_rows(long first, long n, float* out_host) {
    if (first < 0 || n < 0 || first + n > n_) throw std::invalid_argument("gallery: row range outside the gallery");
    if (n > 0) FH_HIP(hipMemcpy(out_host, rows_.as<float>() + (size_t)first * dim_, (size_t)n * dim_ * sizeof(float), hipMemcpyDeviceToHost));
}

// Template pooling.  The host reads src's ids (as remove_ids does), groups them (group_ids.h: the one definition of the grouping) and
// turns the groups into work items of at most `chunk` rows: an identity of one chunk is summed straight into its row, a longer one
// chunk by chunk into scratch partials that a second launch adds in chunk order (gallery_fuse.hip).  Everything is computed before a
// member of this gallery changes.
long Gallery::fuse_from(Gallery& src, bool unit, int chunk) {
    if (dim_ % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    if (src.n_ == 0) {                                           // nothing to read, nothing to launch: the capacity stays
        n_ = 0; base_ = 0; fused_ = true;
        set_live(tags_, false);
        return 0;
    }
    FH_HIP(hipDeviceSynchronize());                              // queued scans of either handle still read what is about to change
    const long n = src.n_;
    std::vector<int> ids((size_t)n), order((size_t)n), uniq((size_t)n);
    std::vector<long long> starts((size_t)n + 1);
    FH_HIP(hipMemcpy(ids.data(), src.ids_.buf.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    const long m = (long)group_ids(ids.data(), n, order.data(), starts.data(), uniq.data());
    if (m <= 0) throw std::runtime_error("gallery: the gallery's ids cannot be grouped (a negative id, or more rows than an int counts)");
    std::vector<FuseItem> items, finish;
    items.reserve((size_t)m);
    int parts = 0;
    for (long j = 0; j < m; ++j) {
        const long b = (long)starts[(size_t)j], cnt = (long)starts[(size_t)j + 1] - b;
        if (cnt <= chunk) { items.push_back({(int)b, (int)cnt, (int)j, 1}); continue; }
        const int first = parts;
        for (long c = 0; c < cnt; c += chunk) items.push_back({(int)(b + c), (int)std::min<long>(chunk, cnt - c), parts++, 0});
        finish.push_back({first, parts - first, (int)j, 1});
    }
    const size_t n1 = items.size(), n2 = finish.size();
    items.insert(items.end(), finish.begin(), finish.end());
    DevBuf d_order, d_items, d_part;
    d_order.ensure((size_t)n * sizeof(int));
    d_items.ensure(items.size() * sizeof(FuseItem));
    if (parts > 0) d_part.ensure((size_t)parts * rows_.row_bytes);
    FH_HIP(hipMemcpy(d_order.p, order.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    FH_HIP(hipMemcpy(d_items.p, items.data(), items.size() * sizeof(FuseItem), hipMemcpyHostToDevice));
    n_ = 0;                                                      // a new row set: labelled, without tags until src's are pooled below
    set_live(ids_, true);
    set_live(tags_, false);
    reserve(m);
    FH_HIP(hipMemcpy(ids_.buf.p, uniq.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice));
    launch_gallery_fuse_sum(src.rows_.as<float>(), d_order.as<int>(), d_items.as<FuseItem>(), (long)n1, dim_, rows_.as<float>(),
                            d_part.as<float>(), unit, nullptr);
    launch_gallery_fuse_sum(d_part.as<float>(), nullptr, d_items.as<FuseItem>() + n1, (long)n2, dim_, rows_.as<float>(), nullptr, unit, nullptr);
    FH_HIP(hipGetLastError());
    FH_HIP(hipDeviceSynchronize());
    n_ = m; base_ = 0; fused_ = true;
    if (src.tags_.live) {                                        // row j carries the OR of the tags of identity j's rows
        DevBuf d_starts;
        d_starts.ensure(((size_t)m + 1) * sizeof(long long));
        FH_HIP(hipMemcpy(d_starts.p, starts.data(), ((size_t)m + 1) * sizeof(long long), hipMemcpyHostToDevice));
        need_tags();                                             // (all ones first: one more pass over m words)
        launch_fuse_tags(src.tags_.as<unsigned>(), d_order.as<int>(), d_starts.as<long long>(), m, tags_.as<unsigned>(), nullptr);
        rebuild_tile_or(0, m);
    }
    if (rows16_.live) convert16(0, m);
    return m;
}

void Gallery::self_scores_dev(const Gallery& tmpl, float* out, hipStream_t s) {
    need_labelled("fh_gallery_self_scores_dev");
    if (!tmpl.fused_)
        throw std::runtime_error("gallery: fh_gallery_self_scores_dev needs a template gallery that fh_gallery_fuse_ids made (and no upload / enroll since)");
    if (n_ == 0) return;
    launch_gallery_self_scores(rows_.as<float>(), ids_.as<int>(), n_, tmpl.rows_.as<float>(), tmpl.ids_.as<int>(), tmpl.n_, dim_, out, s);
    FH_HIP(hipGetLastError());
}

void Gallery::cluster_dev(float thr, int min_pts, bool noise_self, int* labels, int* info, hipStream_t s) {
    if (dim_ % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    if (n_ == 0) {
        if (info) FH_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int), s));
        return;
    }
    if (n_ > (long)INT_MAX) throw std::runtime_error("gallery: row positions must fit in 31 bits");
    cl_deg_.ensure((size_t)n_ * sizeof(int));
    cl_parent_.ensure((size_t)n_ * sizeof(int));
    cl_best_.ensure((size_t)n_ * sizeof(unsigned long long));
    launch_gallery_cluster(rows_.as<float>(), n_, dim_, thr, min_pts, noise_self, cl_deg_.as<int>(), cl_parent_.as<int>(),
                           cl_best_.as<unsigned long long>(), labels, info, s);
    FH_HIP(hipGetLastError());
}

void Gallery::pair_hist_dev(unsigned long long* hist, unsigned long long* nan, hipStream_t s) {
    need_labelled("fh_gallery_pair_hist_dev");
    if (dim_ % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    if (n_ == 0) {
        FH_HIP(hipMemsetAsync(hist, 0, 2 * (size_t)kHistBins * sizeof(unsigned long long), s));
        if (nan) FH_HIP(hipMemsetAsync(nan, 0, 2 * sizeof(unsigned long long), s));
        return;
    }
    if (n_ > (long)INT_MAX) throw std::runtime_error("gallery: row positions must fit in 31 bits");
    cl_hist_.ensure(gallery_pair_hist_scratch_bytes());
    launch_gallery_pair_hist(rows_.as<float>(), ids_.as<int>(), n_, dim_, cl_hist_.as<unsigned long long>(), hist, nan, s);
    FH_HIP(hipGetLastError());
}

void Gallery::pairs_dev(int cls, int side, float thr, int cap, unsigned long long* info, float* out_score, int* out_rows, int* out_ids,
                        hipStream_t s) {
    if (dim_ % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    if (n_ == 0) {
        launch_pairs_empty(cap, info, out_score, out_rows, out_ids, s);
        FH_HIP(hipGetLastError());
        return;
    }
    if (n_ > (long)INT_MAX) throw std::runtime_error("gallery: row positions must fit in 31 bits");
    cl_pairs_.ensure(gallery_pairs_scratch_bytes(cap));
    launch_gallery_pairs(rows_.as<float>(), ids_.live ? ids_.as<int>() : nullptr, n_, dim_, cls, side, thr, cap,
                         cl_pairs_.as<unsigned long long>(), info, out_score, out_rows, out_ids, s);
    FH_HIP(hipGetLastError());
}

void Gallery::set_ids(const int* ids, bool device_src) {
    if (n_ == 0) return;
    FH_HIP(hipDeviceSynchronize());                              // queued scans still read the ids that are about to change
    set_live(ids_, true);
    FH_HIP(hipMemcpy(ids_.buf.p, ids, (size_t)n_ * sizeof(int), device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    fused_ = false;
}

// The host reads the ids and lists the surviving positions in order; compact() moves every live column by that list.  index_base
// stays; the certificate's gallery maxima and bad-value flag stay as they are — an upper bound over a superset of the rows is still an
// upper bound, so F16_RERANK stays exact (a gallery whose only bad row was removed keeps taking the fp32 route until the next upload).
long Gallery::remove_ids(const int* ids_host, long n_ids) {
    need_labelled("fh_gallery_remove_ids");
    if (n_ == 0 || n_ids <= 0) return 0;
    FH_HIP(hipDeviceSynchronize());                              // queued scans still read the buffers that are about to be replaced
    std::vector<int> have((size_t)n_), gone(ids_host, ids_host + n_ids), map;
    FH_HIP(hipMemcpy(have.data(), ids_.buf.p, (size_t)n_ * sizeof(int), hipMemcpyDeviceToHost));
    std::sort(gone.begin(), gone.end());
    map.reserve((size_t)n_);
    for (long r = 0; r < n_; ++r)
        if (!std::binary_search(gone.begin(), gone.end(), have[(size_t)r])) map.push_back((int)r);
    const long m = (long)map.size(), removed = n_ - m;
    if (removed == 0) return 0;
    if (m == 0) { n_ = 0; return removed; }                      // empty again (capacity kept); the next enrol decides the kind afresh
    DevBuf dmap;
    dmap.ensure((size_t)m * sizeof(int));
    FH_HIP(hipMemcpy(dmap.p, map.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice));
    compact(dmap.as<int>(), m);
    if (tags_.live) rebuild_tile_or(0, m);                       // rows moved across tile borders: every tile's OR anew
    return removed;
}

// ------------------------------------------------------------------------------------------ the queries
void Gallery::label_dev(const float* q, const unsigned* masks, int Q, float thr, bool ids, int* out_label, float* out_score, hipStream_t s) {
    if (ids) need_labelled(std::string("fh_gallery_label_ids_") + (masks ? "tagged_dev" : "dev"));
    // the best (admitted) identity is the identity of the best (admitted) row: the k = 1 row call, then a gather of its id
    best_i_.ensure((size_t)std::max(Q, 1) * sizeof(int));
    topk_dev(q, masks, Q, 1, false, out_score, nullptr, best_i_.as<int>(), s);
    if (ids) launch_ids_of_rows(out_score, best_i_.as<int>(), Q, ids_.as<int>(), base_, thr, true, out_label, s);
    else launch_label(out_score, best_i_.as<int>(), Q, thr, out_label, s);
    FH_HIP(hipGetLastError());
}

void Gallery::topk_dev(const float* q, const unsigned* masks, int Q, int k, bool ids, float* out_score, int* out_id, int* out_row, hipStream_t s) {
    if (Q <= 0 || Q > 256 || k <= 0 || k > 16) throw std::runtime_error("gallery: need 0 < Q <= 256 and 0 < k <= 16");
    if (dim_ % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    if (ids) need_labelled(std::string("fh_gallery_topk_ids_") + (masks ? "tagged_dev" : "dev"));
    const bool by_row = ids && k == 1 && !masks;                 // the best identity = the identity of the best row of the scan mode
    if (by_row && !out_row) { best_i_.ensure((size_t)Q * sizeof(int)); out_row = best_i_.as<int>(); }
    // F16_RERANK (gallery_f16.hip): fp16 scan for 32 candidates per query -> exact fp32 re-score + certificate -> the uncertified
    // queries, compacted on the device, through the fp32 scan.  It answers lists of ROWS over ALL rows: the 32 unfiltered candidates
    // certify nothing about a subset of the rows or about an identity list.  Rows with a value the fp16 copy cannot hold (non-finite,
    // > 65504), an empty gallery and dims that are not a multiple of 128 take the fp32 scan for the whole batch as well.
    if (rows16_.live && !masks && (!ids || by_row) && !f16_bad_ && n_ > 0 && dim_ % 128 == 0) {
        topk_f16(q, Q, k, out_score, out_row, s);
    } else {
        if (rows16_.live) host_fallback_ += Q;
        scan_f32(q, masks, Q, k, ids && !by_row, out_score, out_id, out_row, s, nullptr);
    }
    if (by_row) {
        launch_ids_of_rows(out_score, out_row, Q, ids_.as<int>(), base_, 0.f, false, out_id, s);
        FH_HIP(hipGetLastError());
    }
}

void Gallery::topk_f16(const float* q, int Q, int k, float* out_score, int* out_idx, hipStream_t s) {
    const int qrows = (Q + 63) / 64 * 64, KC = GAL16_KC;
    const int parts16 = gallery16_parts(n_, Q, nullptr);
    q16_.ensure((size_t)qrows * dim_ * sizeof(uint16_t));
    ps16_.ensure((size_t)parts16 * Q * KC * sizeof(float));
    pi16_.ensure((size_t)parts16 * Q * KC * sizeof(int));
    seed16_s_.ensure((size_t)Q * KC * sizeof(float));
    seed16_i_.ensure((size_t)Q * KC * sizeof(int));
    cand_s_.ensure((size_t)Q * KC * sizeof(float));
    cand_i_.ensure((size_t)Q * KC * sizeof(int));
    fb_cnt_.ensure(sizeof(int));
    fb_idx_.ensure((size_t)Q * sizeof(int));
    fb_s_.ensure((size_t)Q * k * sizeof(float));
    fb_i_.ensure((size_t)Q * k * sizeof(int));
    FH_HIP(hipMemsetAsync(fb_cnt_.p, 0, sizeof(int), s));
    launch_gallery16_candidates(rows16_.as<uint16_t>(), n_, dim_, q, q16_.as<uint16_t>(), Q, base_, ps16_.as<float>(), pi16_.as<int>(),
                                seed16_s_.as<float>(), seed16_i_.as<int>(), cand_s_.as<float>(), cand_i_.as<int>(), s);
    launch_gallery16_rescore(rows_.as<float>(), n_, dim_, q, Q, k, base_, cand_s_.as<float>(), cand_i_.as<int>(), gbound_[0], gbound_[1],
                             gbound_[2], out_score, out_idx, fb_cnt_.as<int>(), fb_idx_.as<int>(), ctr_.as<unsigned long long>(), s);
    // fall-back: the fp32 scan for the compacted uncertified queries (workgroups beyond the device count exit at once), then scatter
    qpack_.ensure((size_t)qrows * dim_ * sizeof(float));
    launch_gallery16_gather(q, Q, dim_, fb_cnt_.as<int>(), fb_idx_.as<int>(), qpack_.as<float>(), s);
    scan_f32(nullptr, nullptr, Q, k, false, fb_s_.as<float>(), nullptr, fb_i_.as<int>(), s, fb_cnt_.as<int>());
    launch_gallery16_scatter(fb_s_.as<float>(), fb_i_.as<int>(), Q, k, fb_cnt_.as<int>(), fb_idx_.as<int>(), out_score, out_idx, s);
    FH_HIP(hipGetLastError());
}

// queries as the GEMM's N operand: whole 64-row tiles, zero rows behind Q (only that tail is cleared)
void Gallery::pack_queries(const float* q, int Q, hipStream_t s) {
    const int qrows = (Q + 63) / 64 * 64;
    qpack_.ensure((size_t)qrows * dim_ * sizeof(float));
    if (qrows > Q) FH_HIP(hipMemsetAsync(qpack_.as<float>() + (size_t)Q * dim_, 0, (size_t)(qrows - Q) * dim_ * sizeof(float), s));
    FH_HIP(hipMemcpyAsync(qpack_.p, q, (size_t)Q * dim_ * sizeof(float), hipMemcpyDeviceToDevice, s));
}

// The threshold search: the scan with the hit bitmap as its epilogue, counts, lists (gallery_range.hip) — on the fp32 rows always, so
// the answer is the same in either scan mode and the F16_RERANK counters stay as they are.
void Gallery::range_dev(const float* q, const unsigned* masks, int Q, float thr, int cap, long long* counts, float* out_score, int* out_row,
                        int* out_id, hipStream_t s) {
    if (dim_ % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    if (out_id) need_labelled("fh_gallery_range_dev with d_ids");
    if (masks && n_ > 0) need_tags();
    pack_queries(q, Q, s);
    rg_hits_.ensure(gallery_range_hits_bytes(n_, Q));
    rg_units_.ensure(gallery_range_units_bytes(n_, Q));
    launch_gallery_range(rows_.as<float>(), n_, dim_, qpack_.as<float>(), tags_.as<unsigned>(), masks, Q, base_, thr, cap,
                         rg_hits_.as<unsigned>(), rg_units_.as<int>(), out_id ? ids_.as<int>() : nullptr, counts, out_score, out_row, out_id, s);
    FH_HIP(hipGetLastError());
}

// The deep top-k: the scan with the block maxima as its epilogue, then blocks, rows and lists (gallery_deep.hip) — on the fp32 rows
// always, as the threshold search; its only scratch is its own.
void Gallery::topk_deep_dev(const float* q, const unsigned* masks, int Q, int k, float* out_score, int* out_row, int* out_id, hipStream_t s) {
    if (dim_ % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    if (out_id) need_labelled("fh_gallery_topk_deep_dev with d_ids");
    if (masks && n_ > 0) need_tags();
    pack_queries(q, Q, s);
    dp_bmax_.ensure(gallery_deep_bmax_bytes(n_, Q));
    dp_bmax_t_.ensure(gallery_deep_bmax_t_bytes(n_, Q));
    dp_chosen_.ensure(gallery_deep_chosen_bytes(Q, k));
    dp_cand_.ensure(gallery_deep_cand_bytes(Q, k));
    launch_gallery_deep(rows_.as<float>(), n_, dim_, qpack_.as<float>(), tags_.as<unsigned>(), masks, Q, base_, k, dp_bmax_.as<float>(),
                        dp_bmax_t_.as<float>(), dp_chosen_.as<int>(), dp_cand_.as<float>(), out_id ? ids_.as<int>() : nullptr, out_score,
                        out_row, out_id, s);
    FH_HIP(hipGetLastError());
}

// ONE pass over the gallery: dot products stay in the MFMA accumulators, per-workgroup top-k lists come out and are merged
// (gallery_scan.h).  masks: only each query's admitted rows; ids: lists of identities (out_id; out_row may be null); qcount (device,
// the F16_RERANK fall-back): only that many queries are live, and the scan runs unseeded.
void Gallery::scan_f32(const float* q, const unsigned* masks, int Q, int k, bool ids, float* out_score, int* out_id, int* out_row, hipStream_t s,
                       const int* qcount) {
    if (masks && n_ > 0) need_tags();
    if (q) pack_queries(q, Q, s);
    // part planes [gallery_parts][Q][k] and seed planes [Q][k] (ids: with their identity planes)
    const int parts = n_ > 0 ? gallery_parts(n_, Q, nullptr) : 0;
    const size_t plane = (size_t)std::max(parts, 1) * Q * k, seed = (size_t)Q * k;
    ps_.ensure(plane * sizeof(float));
    pi_.ensure(plane * sizeof(int));
    seed_s_.ensure(seed * sizeof(float));
    seed_i_.ensure(seed * sizeof(int));
    if (ids) { pd_.ensure(plane * sizeof(int)); seed_d_.ensure(seed * sizeof(int)); }
    GalArgs a{};
    a.gal = rows_.buf.p; a.q = qpack_.p; a.idx_base = base_; a.dim = dim_; a.Q = Q; a.k = k;
    a.ps = ps_.as<float>(); a.pi = pi_.as<int>(); a.qcount = qcount;
    if (ids) { a.ids = ids_.as<int>(); a.pd = pd_.as<int>(); }
    if (masks) { a.tags = tags_.as<unsigned>(); a.qmask = masks; a.tile_or = tile_or_.as<unsigned>(); a.tag_ctr = tag_ctr_.as<unsigned long long>(); }
    launch_gallery_scan(a, n_, qcount ? nullptr : seed_s_.as<float>(), qcount ? nullptr : seed_i_.as<int>(), ids ? seed_d_.as<int>() : nullptr, s);
    if (ids) launch_topk_merge_ids(ps_.as<float>(), pd_.as<int>(), pi_.as<int>(), parts, Q, k, out_score, out_id, out_row, s);
    else launch_topk_merge(ps_.as<float>(), pi_.as<int>(), parts, Q, k, out_score, out_row, s, qcount);
    FH_HIP(hipGetLastError());
}

}  // namespace fh
