// roc_plan.h — the ONE definition of how pair scores are binned (fh_hist_bin, and through it the histogram epilogue of
// gallery_cluster.hip behind fh_gallery_pair_hist_dev) and of how an operating threshold is read off a genuine / impostor histogram
// (fh_roc_from_hist).  Host code, no GPU, no HIP header: a stand-alone program can include it (tests/native/roc_plan_sanitize.cpp); the
// bin rule alone is also compiled for the device, behind FH_ROC_HD.
//   bins     kHistBins = 2048 over the mapped score.  With t = s * 2048.0f (a power of two: exact, but for an overflow to +-inf, which
//            lands where it should) hist_bin(s) is -1 for a NaN, 0 for t <= 1, 2047 for t > 2047 (+inf too), (int)ceilf(t) - 1 otherwise.
//            Bin b holds b/2048 < s <= (b+1)/2048; bin 0 also holds everything at or below 1/2048 (scores <= 0, -inf), bin 2047
//            everything above 2047/2048 (a score a hair above 1).
//   property the half-open side is the library's strict test: for every b in 1..2047, b/2048 is an exact fp32 value and
//                A[b] = sum over b' >= b of h[b']  ==  the number of binned scores with s > b/2048,
//            i.e. exactly the pairs that `score > threshold` accepts at threshold = b/2048.  A[0] counts every non-NaN score.
//   roc      hist[2][2048]: plane 0 genuine, plane 1 impostor; N_g, N_i = the plane sums (they must fit in 64 bits: the pairs of one
//            gallery always do).  out[0] = the operating point of max_far: the smallest b in 1..2047 with
//            A_i[b] <= (uint64_t)floor(max_far * (double)N_i) — the one floating-point step, everything else is uint64_t / __int128.
//            out[1] = the equal-error point: the smallest b in 1..2047 with FAR_b <= FRR_b, decided as
//            A_i[b] * N_g <= (N_g - A_g[b]) * N_i in unsigned __int128.  A point is {b / 2048.0f, b, A_g[b], A_i[b], N_g, N_i}; one for
//            which no b exists is {1.0f, -1, 0, 0, N_g, N_i}.
//            Returns 0, or -1 — nothing written — for a null pointer, max_far outside [0, 1] or NaN, N_g == 0 or N_i == 0.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FH_ROC_HD __host__ __device__
#else
#define FH_ROC_HD
#endif

namespace fh {

constexpr int kHistBins = 2048;

struct RocPoint {
    float threshold;
    int32_t bin;
    uint64_t true_accepts, false_accepts, genuine, impostor;
};

FH_ROC_HD inline int hist_bin(float s) {
    const float t = s * 2048.0f;
    if (t != t) return -1;
    if (t <= 1.0f) return 0;
    if (t > 2047.0f) return kHistBins - 1;
    return (int)ceilf(t) - 1;
}

inline int roc_from_hist(const uint64_t* hist, double max_far, RocPoint out[2]) {
    if (!hist || !out || !(max_far >= 0.0 && max_far <= 1.0)) return -1;
    uint64_t n_g = 0, n_i = 0;
    for (int b = 0; b < kHistBins; ++b) { n_g += hist[b]; n_i += hist[kHistBins + b]; }
    if (n_g == 0 || n_i == 0) return -1;
    // the documented floor; (double)n_i may round up to 2^64, which no uint64_t holds: every A_i is below that bound anyway
    const double lim = std::floor(max_far * (double)n_i);
    const uint64_t allowed = lim >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)lim;
    RocPoint pt[2] = {{1.0f, -1, 0, 0, n_g, n_i}, {1.0f, -1, 0, 0, n_g, n_i}};
    uint64_t a_g = n_g - hist[0], a_i = n_i - hist[kHistBins];           // A[1]
    for (int b = 1; b < kHistBins; ++b) {
        const bool ok[2] = {a_i <= allowed,
                            (unsigned __int128)a_i * n_g <= (unsigned __int128)(n_g - a_g) * n_i};
        for (int k = 0; k < 2; ++k)
            if (pt[k].bin < 0 && ok[k]) pt[k] = {(float)b / 2048.0f, b, a_g, a_i, n_g, n_i};
        a_g -= hist[b]; a_i -= hist[kHistBins + b];                      // A[b + 1]
    }
    out[0] = pt[0]; out[1] = pt[1];
    return 0;
}

}  // namespace fh
