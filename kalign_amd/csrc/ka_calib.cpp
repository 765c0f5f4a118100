// ka_calib.cpp -- the calibration metrics of (confidence, correct) pairs: brier_score, expected_calibration_error and
// calibration_curve of the reference's benchmarks/downstream/calibration.py, per segment of the items and over their pool
// (_aggregate_summary pools its cases in case order).  Host only, the standard library only: nothing here includes a
// device header, so the unit compiles and runs on its own (a main that defines fail()).
//
// The reference's order of operations is kept: serial double sums in item order, b = (int)(p * n_bins) clamped to the last
// bin, a bin's two means divided before they are subtracted, the weight count / n divided before it is multiplied.  No
// product may be contracted into a sum (the library is built with -ffp-contract=off; the pragma below says so here).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "kalign_amd.h"

// the thread's error text (ka_last_error): defined in ka_api.cpp
__attribute__((visibility("hidden"))) int fail(const std::string& m);

namespace {

// one slot: the items lo .. hi - 1
void calib_slot(const double* p, const uint8_t* o, long long lo, long long hi, int n_bins, std::vector<double>& conf, std::vector<double>& corr,
                double* brier, double* ece, double* frac, long long* counts)
{
#pragma clang fp contract(off)
        const long long n = hi - lo;
        std::vector<long long> cnt(n_bins, 0);
        conf.assign(n_bins, 0.0);
        corr.assign(n_bins, 0.0);
        double total = 0.0;
        for (long long k = lo; k < hi; k++) {
                const double x = p[k], y = (double)o[k], d = x - y;
                total += d * d;
                int b = (int)(x * (double)n_bins);
                if (b >= n_bins) b = n_bins - 1;
                conf[b] += x;
                corr[b] += y;
                cnt[b]++;
        }
        double e = 0.0;
        for (int b = 0; b < n_bins; b++) {
                double fc = std::numeric_limits<double>::quiet_NaN();
                if (cnt[b] > 0) {
                        const double avg = conf[b] / (double)cnt[b];
                        fc = corr[b] / (double)cnt[b];
                        const double w = (double)cnt[b] / (double)n;
                        e += w * std::fabs(avg - fc);
                }
                if (frac) frac[b] = fc;
                if (counts) counts[b] = cnt[b];
        }
        if (brier) *brier = n ? total / (double)n : 0.0;
        if (ece) *ece = n ? e : 0.0;
}

} // namespace

extern "C" int ka_calibration(int n_seg, const long long* seg_first, const double* predicted, const uint8_t* actual, int n_bins, double* brier,
                              double* ece, double* bin_fraction, long long* bin_counts)
{
        if (n_seg < 0 || !seg_first) return fail("ka_calibration: bad arguments");
        if (n_bins < 1) return fail("ka_calibration: n_bins " + std::to_string(n_bins) + " < 1");
        if (seg_first[0] != 0) return fail("ka_calibration: seg_first does not ascend from 0 (segment 0 starts at " + std::to_string(seg_first[0]) + ")");
        for (int s = 0; s < n_seg; s++)
                if (seg_first[s + 1] < seg_first[s])
                        return fail("ka_calibration: seg_first does not ascend from 0 (segment " + std::to_string(s) + " ends before it starts)");
        const long long n = seg_first[n_seg];
        if (n > 0 && (!predicted || !actual)) return fail("ka_calibration: bad arguments");
        for (long long k = 0; k < n; k++) {
                if (!(predicted[k] >= 0.0 && predicted[k] <= 1.0)) {     // (NaN fails both)
                        char v[40];
                        snprintf(v, sizeof v, "%.17g", predicted[k]);
                        return fail("ka_calibration: item " + std::to_string(k) + ": predicted " + v + " is not in [0, 1]");
                }
                if (actual[k] > 1)
                        return fail("ka_calibration: item " + std::to_string(k) + ": actual " + std::to_string((int)actual[k]) + " is neither 0 nor 1");
        }
        std::vector<double> conf, corr;
        for (int s = 0; s <= n_seg; s++) {
                const long long lo = s < n_seg ? seg_first[s] : 0, hi = s < n_seg ? seg_first[s + 1] : n;
                calib_slot(predicted, actual, lo, hi, n_bins, conf, corr, brier ? brier + s : nullptr, ece ? ece + s : nullptr,
                           bin_fraction ? bin_fraction + (size_t)s * n_bins : nullptr, bin_counts ? bin_counts + (size_t)s * n_bins : nullptr);
        }
        return KA_OK;
}
