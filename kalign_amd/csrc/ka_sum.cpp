// ka_sum.cpp -- host side of the summaries and trimming of finished rows (kalign.utils: alignment_stats,
// consensus_sequence, remove_gap_columns, trim_alignment, pairwise_identity_matrix) for a batch of families: the ka_sum_fam
// handle of the C ABI.  One alignment is a batch of one.
//
// The rows are packed as ka_batch_rows hands them out (a row of W columns W + 1 bytes) and uploaded in one copy; the
// column table (ka_sum.hip) is built once at create, with every family's exact sums and its character-presence mask.  The
// device returns exact integers; the doubles are computed here, each the one division of two of those integers
// (ka_sum_finish), and the two threshold comparisons on the device are the same divisions of the same integers.
//
// The gap structure (the reference's benchmarks/analysis.py: compute_gap_stats) and the rows without their gaps (dealign_msa)
// come from a walk along rows: ka_sum_fam_gaps, ka_sum_fam_ungapped.  The row records and the families' exact sums come
// back once and stay on the host; the doubles are computed here alone (gap_finish, which ka_sum_fam_gap_values hands out).
//
// Every check runs on the host before anything is launched (sum_fam_check; ka_sum_fam_check is its public form; the rule
// of a consensus, keep or compact call: thresholds, rule): a refused call launches nothing and leaves the handle usable.
#include <memory>
#include "ka_ctx.h"
#include "ka_sum.h"

namespace {

int sum_fam_check(const char* who, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens)
{
        const std::string me(who);
        if (!rows || !alnlens) return fail(me + ": bad arguments");
        if (ka_fam_check_first(me, n_fam, fam_first)) return KA_FAIL;
        long long cols = 0, items = 0;
        for (int f = 0; f < n_fam; f++) {
                const std::string fam = me + ": family " + std::to_string(f);
                const long long N = fam_first[f + 1] - fam_first[f], W = alnlens[f];
                if (W < 1) return fail(fam + ": alnlen " + std::to_string(W));
                if (N * W > INT32_MAX)
                        return fail(fam + ": " + std::to_string(N) + " rows of " + std::to_string(W) + " columns; a family holds fewer than 2^31 cells");
                cols += W;
                items += N * ((W + KA_SUM_CHUNK) / KA_SUM_CHUNK);
                if (cols > INT32_MAX) return fail(me + ": more than 2^31 - 1 columns in the batch");
                if (items > INT32_MAX) return fail(me + ": more than 2^31 - 1 row chunks in the batch");
        }
        return KA_OK;
}

// the entries of each of the three identity matrices of a batch, the sum of N_f^2, or -1 (ka_sum_fam_identity_entries is
// its public form; ka_sum_fam_identity runs it over the handle's families before anything is launched)
long long idm_entries(const char* who, int n_fam, const int* fam_first)
{
        const std::string me(who);
        if (ka_fam_check_first(me, n_fam, fam_first)) return -1;
        long long sum = 0;
        for (int f = 0; f < n_fam; f++) {
                const long long N = fam_first[f + 1] - fam_first[f];
                sum += N * N;                                    // (N < 2^31 and the sum so far < 2^31: no overflow)
                if (sum > INT32_MAX)
                        return fail(me + ": family " + std::to_string(f) + ": " + std::to_string(N) + " rows bring the matrices to " + std::to_string(sum) +
                                    " entries; a batch holds fewer than 2^31"), -1;
        }
        return sum;
}

// the doubles of one family from its exact counts (counts[6] as ka_sum_fam_summary lays them out), each the one division
// kalign.utils.alignment_stats makes.  The one place these expressions live.
void ka_sum_finish(const long long* counts, double* values)
{
        values[0] = (double)counts[0] / (double)counts[1];
        values[1] = (double)counts[2] / (double)counts[3];
        values[2] = counts[5] > 0 ? (double)counts[4] / (double)counts[5] : 0.0;
}

// the seven doubles of one family's gap structure from its eight exact counts (ka_sum_fam_gaps' layout), each as the
// reference's compute_gap_stats divides: the expansion factor is the width over the ROUNDED mean length, two roundings; a
// zero denominator gives 0.0.  The one place these expressions live.
void gap_finish(const long long* c, double* v)
{
        const double N = (double)c[0], W = (double)c[1];
        v[0] = c[0] > 0 ? (double)c[2] / N : 0.0;
        v[1] = v[0] > 0.0 ? W / v[0] : 0.0;
        v[2] = c[0] * c[1] > 0 ? (double)c[3] / (double)(c[0] * c[1]) : 0.0;
        v[3] = c[4] > 0 ? (double)c[3] / (double)c[4] : 0.0;
        v[4] = c[0] > 0 ? (double)c[5] / N : 0.0;
        v[5] = c[0] > 0 ? (double)c[6] / N : 0.0;
        v[6] = c[1] > 0 ? (double)c[7] / W : 0.0;
}

// 'N' when every character of the family, upper-cased, lies in ATCGUN, else 'X' (consensus_sequence's heuristic)
uint8_t ambiguous_of(const unsigned* present)
{
        for (int b = 0; b < 256; b++) {
                if (!(present[b >> 5] >> (b & 31) & 1u)) continue;
                const int u = b >= 'a' && b <= 'z' ? b - 32 : b;
                if (!std::strchr("ATCGUN", u) || !u) return 'X';
        }
        return 'N';
}

} // namespace

struct ka_sum_fam : KaStage {
        uint8_t gap = '-';
        int nFam = 0, cols = 0, nTiles = 0, nItems = 0;
        long long bytes = 0;                   // of the packed rows
        std::vector<KaSumFam> fams;
        std::vector<unsigned long long> famSums;
        std::vector<uint8_t> ambiguous;
        std::vector<double> hThr;              // a call's rule as it is uploaded
        std::vector<long long> hMaskOff;
        std::vector<int> newW;                 // of the last compact
        long long outBytes = -1;               // of its rows (-1: none)
        DevBuf<KaSumFam> dFams;
        DevBuf<int> dFirst, dNGap, dNDistinct, dTopCount, dKeep, dSrc, dNewW, dMasks;
        DevBuf<uint8_t> dRows, dTopChar, dAmbiguous, dCons, dOut;
        DevBuf<long long> dSame, dMaskOff, dOutOff;
        DevBuf<unsigned long long> dFamSums;
        DevBuf<unsigned> dPresent;
        DevBuf<double> dThr;
        // device ms [0..3]; [4], [5] are the counters of the last call that launches (create, consensus, keep, compact: begin()).
        // The hand-outs (columns, summary, rows) are copies and leave the counters as they are.
        double st[KA_SUM_STATS] = {};
        // the identity matrices: computed by the first ka_sum_fam_identity, then kept on the device
        bool haveIdm = false;
        long long idmEntries = 0;
        DevBuf<int> dIdmFirst, dMatches, dCompared;
        DevBuf<unsigned> dIdmTiles;
        DevBuf<double> dIdentity;
        double idmSt[KA_SUM_IDM_STATS] = {};   // device ms, launches and waits of the call that computed them
        // the gap structure: the row records and the families' sums are computed by the first ka_sum_fam_gaps or
        // ka_sum_fam_ungapped and kept on the host, the ungapped rows by the first ka_sum_fam_ungapped and kept on the device
        bool haveGaps = false, haveUngap = false;
        int numseq = 0;
        std::vector<int> rowFirst, gapRecs;                      // [nFam + 1]; [numseq][KA_SUM_ROWREC]
        std::vector<unsigned long long> gapSums;                 // [nFam][KA_SUM_GAPSUMS]
        std::vector<long long> ungapOff;                         // [numseq + 1]: where a row's characters start
        DevBuf<int> dRowFirst, dGapRecs;
        DevBuf<unsigned long long> dGapSums;
        DevBuf<long long> dUngapOff;
        DevBuf<uint8_t> dUngap;
        double gapSt[KA_SUM_GAP_STATS] = {};   // ka_sum_fam_gap_stats

        KaSumTab tab() const
        {
                KaSumTab a{};
                a.nFam = nFam; a.cols = cols; a.nTiles = nTiles; a.nItems = nItems; a.gap = gap;
                a.fams = dFams.p; a.tileFirst = dFirst.p; a.colFirst = dFirst.p + nFam + 1; a.itemFirst = dFirst.p + 2 * (nFam + 1);
                a.rows = dRows.p;
                a.nGap = dNGap.p; a.nDistinct = dNDistinct.p; a.topCount = dTopCount.p; a.topChar = dTopChar.p; a.samePairs = dSame.p;
                a.famSums = dFamSums.p; a.present = dPresent.p;
                a.thr = dThr.p; a.ambiguous = dAmbiguous.p;
                a.keep = dKeep.p; a.src = dSrc.p; a.newW = dNewW.p; a.outOff = dOutOff.p; a.out = dOut.p;
                return a;
        }
        int create(const char* who, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens);
        // one threshold per family in [0, 1] (NULL: dflt for every family) to the device
        int thresholds(const char* who, const char* what, const double* thr, double dflt);
        // the column rule of keep and compact, checked and uploaded; *masked: the table carries masks
        int rule(const char* who, const double* gapThr, const int* masks, const long long* maskOff, bool* masked);
        int identity(const char* who, int* matchesOut, int* comparedOut, double* identityOut);
        KaGapTab gapTab() const
        {
                KaGapTab a{};
                a.nFam = nFam; a.nRows = numseq; a.cols = cols; a.gap = gap;
                a.fams = dFams.p; a.rowFirst = dRowFirst.p; a.colFirst = dFirst.p + nFam + 1; a.rows = dRows.p; a.nGap = dNGap.p;
                a.recs = dGapRecs.p; a.sums = dGapSums.p; a.off = dUngapOff.p; a.out = dUngap.p;
                return a;
        }
        long long characters() const;          // of the batch, from the column table's sums: nothing is launched
        int gaps(const char* who);             // the row pass and the gappy pass, once
        int ungapped(const char* who, uint8_t* out, long long cap, long long* rowOffOut);
};

int ka_sum_fam::create(const char* who, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens)
{
        const std::string me(who);
        nFam = n_fam;
        fams.assign(nFam, KaSumFam{});
        std::vector<int> first((size_t)3 * (nFam + 1), 0);       // tiles, columns, gather items
        for (int f = 0; f < nFam; f++) {
                KaSumFam& d = fams[f];
                d.N = fam_first[f + 1] - fam_first[f]; d.W = alnlens[f];
                d.firstCol = cols; d.chunks = (d.W + KA_SUM_CHUNK) / KA_SUM_CHUNK; d.rowOff = bytes;
                first[f] = nTiles; first[nFam + 1 + f] = cols; first[2 * (nFam + 1) + f] = nItems;
                nTiles += (d.W + KA_SUM_TILE - 1) / KA_SUM_TILE;
                cols += d.W;
                nItems += d.N * d.chunks;
                bytes += (long long)d.N * (d.W + 1);
                numseq += d.N;
        }
        first[nFam] = nTiles; first[2 * nFam + 1] = cols; first[3 * nFam + 2] = nItems;
        famSums.assign((size_t)nFam * KA_SUM_FAMSUMS, 0);
        std::vector<unsigned> present((size_t)nFam * 8, 0);
        if (open(2)) return KA_FAIL;
        if (dFams.alloc(nFam) || dFirst.alloc(first.size()) || dRows.alloc((size_t)bytes) || dNGap.alloc(cols) || dNDistinct.alloc(cols) ||
            dTopCount.alloc(cols) || dTopChar.alloc(cols) || dSame.alloc(cols) || dFamSums.alloc(famSums.size()) || dPresent.alloc(present.size()) ||
            dThr.alloc(nFam) || dAmbiguous.alloc(nFam) || dMaskOff.alloc(nFam) || dKeep.alloc(cols) || dSrc.alloc(cols) || dNewW.alloc(nFam) ||
            dOutOff.alloc(nFam) || dCons.alloc((size_t)cols + nFam) || dOut.alloc((size_t)bytes))
                return fail(me + ": out of device memory");
        HIPCHK(hipMemcpyAsync(dFams.p, fams.data(), sizeof(KaSumFam) * nFam, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dFirst.p, first.data(), sizeof(int) * first.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dRows.p, rows, (size_t)bytes, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemsetAsync(dFamSums.p, 0, sizeof(unsigned long long) * famSums.size(), stream));
        HIPCHK(hipMemsetAsync(dPresent.p, 0, sizeof(unsigned) * present.size(), stream));
        HIPCHK(hipEventRecord(ev[0], stream));
        begin();
        if (ka_sum_run_columns(tab(), stream, &nLaunch)) return fail(me + ": the column table's LDS was refused");
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], stream));
        HIPCHK(hipMemcpyAsync(famSums.data(), dFamSums.p, sizeof(unsigned long long) * famSums.size(), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(present.data(), dPresent.p, sizeof(unsigned) * present.size(), hipMemcpyDeviceToHost, stream));
        if (wait()) return KA_FAIL;
        st[0] = ms();
        ambiguous.resize(nFam);
        for (int f = 0; f < nFam; f++) ambiguous[f] = ambiguous_of(&present[(size_t)f * 8]);
        HIPCHK(hipMemcpyAsync(dAmbiguous.p, ambiguous.data(), (size_t)nFam, hipMemcpyHostToDevice, stream));
        return KA_OK;
}

int ka_sum_fam::thresholds(const char* who, const char* what, const double* thr, double dflt)
{
        if (thr)
                for (int f = 0; f < nFam; f++)
                        if (!(thr[f] >= 0.0 && thr[f] <= 1.0))
                                return fail(std::string(who) + ": family " + std::to_string(f) + ": " + what + " " + std::to_string(thr[f]) + " is not in [0, 1]");
        hThr.assign(nFam, dflt);
        if (thr) hThr.assign(thr, thr + nFam);
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipMemcpyAsync(dThr.p, hThr.data(), sizeof(double) * nFam, hipMemcpyHostToDevice, stream));
        return KA_OK;
}

int ka_sum_fam::rule(const char* who, const double* gapThr, const int* masks, const long long* maskOff, bool* masked)
{
        const std::string me(who);
        HIPCHK(hipSetDevice(device));                            // (before anything is allocated: the caller's thread may be on another device)
        std::vector<long long>& off = hMaskOff;
        off.assign(nFam, -1);
        long long n = 0;                                         // ints of `masks` in use
        if (masks && maskOff)
                for (int f = 0; f < nFam; f++) {
                        if (maskOff[f] < 0) continue;
                        if (maskOff[f] + fams[f].W > cols)
                                return fail(me + ": family " + std::to_string(f) + ": mask offset " + std::to_string(maskOff[f]) + " with " +
                                            std::to_string(fams[f].W) + " columns passes the end of the masks (" + std::to_string(cols) + " ints at most)");
                        off[f] = maskOff[f];
                        n = std::max(n, maskOff[f] + fams[f].W);
                }
        *masked = n > 0;
        if (thresholds(who, "gap threshold", gapThr, 1.0)) return KA_FAIL;   // (a refused call has touched no buffer)
        if (n && dMasks.alloc((size_t)n)) return fail(me + ": out of device memory");
        if (n) HIPCHK(hipMemcpyAsync(dMasks.p, masks, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dMaskOff.p, off.data(), sizeof(long long) * nFam, hipMemcpyHostToDevice, stream));
        return KA_OK;                                            // (the caller's and the handle's arrays are read until the call's synchronisation)
}

extern "C" int ka_sum_fam_check(int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens)
{
        return sum_fam_check("ka_sum_fam_check", n_fam, fam_first, rows, alnlens);
}

// the check under another stage's name (library-internal: ka_out.cpp)
int ka_sum_check_named(const std::string& me, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens)
{
        return sum_fam_check(me.c_str(), n_fam, fam_first, rows, alnlens);
}

extern "C" int ka_sum_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens, int gap_char, ka_sum_fam** out)
{
        if (!ctx || !out || gap_char < 0 || gap_char > 255) return fail("ka_sum_fam_create: bad arguments");
        *out = nullptr;
        if (sum_fam_check("ka_sum_fam_create", n_fam, fam_first, rows, alnlens)) return KA_FAIL;
        std::unique_ptr<ka_sum_fam> h(new ka_sum_fam);
        if (h->attach(ctx)) return fail("ka_sum_fam_create: bad context");
        h->gap = (uint8_t)gap_char;
        if (h->create("ka_sum_fam_create", n_fam, fam_first, rows, alnlens)) return KA_FAIL;
        *out = h.release();
        return KA_OK;
}

extern "C" void ka_sum_fam_destroy(ka_sum_fam* h)
{
        ka_stage_destroy(h);
}

extern "C" int ka_sum_fam_columns(ka_sum_fam* h, int* n_gap, int* n_distinct, uint8_t* top_char, int* top_count, long long* same_pairs)
{
        if (!h) return fail("ka_sum_fam_columns: bad arguments");
        HIPCHK(hipSetDevice(h->device));
        const size_t n = (size_t)h->cols;
        if (n_gap) HIPCHK(hipMemcpyAsync(n_gap, h->dNGap.p, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
        if (n_distinct) HIPCHK(hipMemcpyAsync(n_distinct, h->dNDistinct.p, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
        if (top_char) HIPCHK(hipMemcpyAsync(top_char, h->dTopChar.p, n, hipMemcpyDeviceToHost, h->stream));
        if (top_count) HIPCHK(hipMemcpyAsync(top_count, h->dTopCount.p, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
        if (same_pairs) HIPCHK(hipMemcpyAsync(same_pairs, h->dSame.p, sizeof(long long) * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return KA_OK;
}

extern "C" int ka_sum_fam_summary(ka_sum_fam* h, long long* counts_out, double* values_out)
{
        if (!h) return fail("ka_sum_fam_summary: bad arguments");
        for (int f = 0; f < h->nFam; f++) {
                const unsigned long long* s = &h->famSums[(size_t)f * KA_SUM_FAMSUMS];
                const KaSumFam& d = h->fams[f];
                const long long counts[6] = { (long long)s[KA_SUM_GAPS], (long long)d.N * d.W, (long long)s[KA_SUM_CONSERVED], d.W,
                                              (long long)s[KA_SUM_MATCHING], (long long)s[KA_SUM_COMPARED] };
                if (counts_out) std::copy_n(counts, 6, counts_out + (size_t)f * 6);
                if (values_out) ka_sum_finish(counts, values_out + (size_t)f * 3);
        }
        return KA_OK;
}

extern "C" int ka_sum_fam_consensus(ka_sum_fam* h, const double* thresholds, uint8_t* out, uint8_t* ambiguous_out)
{
        if (!h) return fail("ka_sum_fam_consensus: bad arguments");
        h->begin();
        if (h->thresholds("ka_sum_fam_consensus", "threshold", thresholds, 0.5)) return KA_FAIL;
        HIPCHK(hipEventRecord(h->ev[0], h->stream));
        KaSumTab a = h->tab();
        a.out = h->dCons.p;
        ka_sum_run_consensus(a, h->stream, &h->nLaunch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev[1], h->stream));
        if (out) HIPCHK(hipMemcpyAsync(out, h->dCons.p, (size_t)h->cols + h->nFam, hipMemcpyDeviceToHost, h->stream));
        if (h->wait()) return KA_FAIL;
        h->st[1] = h->ms();
        if (ambiguous_out) std::copy(h->ambiguous.begin(), h->ambiguous.end(), ambiguous_out);
        return KA_OK;
}

extern "C" int ka_sum_fam_keep(ka_sum_fam* h, const double* gap_thresholds, const int* masks, const long long* mask_off, int* keep_out, int* new_alnlens)
{
        if (!h) return fail("ka_sum_fam_keep: bad arguments");
        h->begin();
        bool masked = false;
        if (h->rule("ka_sum_fam_keep", gap_thresholds, masks, mask_off, &masked)) return KA_FAIL;
        HIPCHK(hipEventRecord(h->ev[0], h->stream));
        KaSumTab a = h->tab();
        if (masked) { a.masks = h->dMasks.p; a.maskOff = h->dMaskOff.p; }
        ka_sum_run_keep(a, h->stream, &h->nLaunch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev[1], h->stream));
        if (keep_out) HIPCHK(hipMemcpyAsync(keep_out, h->dKeep.p, sizeof(int) * (size_t)h->cols, hipMemcpyDeviceToHost, h->stream));
        if (new_alnlens) HIPCHK(hipMemcpyAsync(new_alnlens, h->dNewW.p, sizeof(int) * h->nFam, hipMemcpyDeviceToHost, h->stream));
        if (h->wait()) return KA_FAIL;
        h->st[2] = h->ms();
        return KA_OK;
}

extern "C" int ka_sum_fam_compact(ka_sum_fam* h, const double* gap_thresholds, const int* masks, const long long* mask_off, int* new_alnlens)
{
        if (!h) return fail("ka_sum_fam_compact: bad arguments");
        h->begin();
        bool masked = false;
        if (h->rule("ka_sum_fam_compact", gap_thresholds, masks, mask_off, &masked)) return KA_FAIL;
        h->outBytes = -1;
        h->newW.assign(h->nFam, 0);
        HIPCHK(hipEventRecord(h->ev[0], h->stream));
        KaSumTab a = h->tab();
        if (masked) { a.masks = h->dMasks.p; a.maskOff = h->dMaskOff.p; }
        ka_sum_run_keep(a, h->stream, &h->nLaunch);
        ka_sum_run_gather(a, h->stream, &h->nLaunch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev[1], h->stream));
        HIPCHK(hipMemcpyAsync(h->newW.data(), h->dNewW.p, sizeof(int) * h->nFam, hipMemcpyDeviceToHost, h->stream));
        if (h->wait()) return KA_FAIL;
        h->st[3] = h->ms();
        long long bytes = 0;
        for (int f = 0; f < h->nFam; f++) bytes += (long long)h->fams[f].N * (h->newW[f] + 1);
        h->outBytes = bytes;
        if (new_alnlens) std::copy(h->newW.begin(), h->newW.end(), new_alnlens);
        return KA_OK;
}

extern "C" long long ka_sum_fam_rows_size(ka_sum_fam* h)
{
        return h ? h->outBytes : -1;
}

extern "C" int ka_sum_fam_rows(ka_sum_fam* h, uint8_t* out, long long cap)
{
        if (!h || !out) return fail("ka_sum_fam_rows: bad arguments");
        if (h->outBytes < 0) return fail("ka_sum_fam_rows: no compacted rows (ka_sum_fam_compact first)");
        if (cap < h->outBytes)
                return fail("ka_sum_fam_rows: " + std::to_string(cap) + " bytes do not hold the rows (" + std::to_string(h->outBytes) + ")");
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipMemcpyAsync(out, h->dOut.p, (size_t)h->outBytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return KA_OK;
}

// The tile table of the batch -- per family the tiles (bi, bj), bi <= bj, of ceil(N / T) tiles a side, tile row after tile
// row -- and one launch over it; then the copies the caller asked for and the call's one wait.  Matrices that are already on
// the device are only copied.
int ka_sum_fam::identity(const char* who, int* matchesOut, int* comparedOut, double* identityOut)
{
        const std::string me(who);
        std::vector<int> first;                                  // (read by the upload until the wait below)
        std::vector<unsigned> tiles;
        int launches = 0;
        const bool compute = !haveIdm;
        HIPCHK(hipSetDevice(device));
        if (compute) {
                std::vector<int> famFirst(nFam + 1, 0);
                for (int f = 0; f < nFam; f++) famFirst[f + 1] = famFirst[f] + fams[f].N;
                idmEntries = idm_entries(who, nFam, famFirst.data());
                if (idmEntries < 0) return KA_FAIL;
                first.assign((size_t)2 * (nFam + 1), 0);         // tiles, entries
                long long ent = 0;
                for (int f = 0; f < nFam; f++) {
                        const int nt = (fams[f].N + KA_SUM_IDM_T - 1) / KA_SUM_IDM_T;
                        first[f] = (int)tiles.size(); first[nFam + 1 + f] = (int)ent;
                        for (int bi = 0; bi < nt; bi++)
                                for (int bj = bi; bj < nt; bj++) tiles.push_back((unsigned)bi << 16 | (unsigned)bj);
                        ent += (long long)fams[f].N * fams[f].N;
                }
                first[nFam] = (int)tiles.size(); first[2 * nFam + 1] = (int)ent;
                if (dIdmFirst.alloc(first.size()) || dIdmTiles.alloc(tiles.size()) || dMatches.alloc((size_t)idmEntries) ||
                    dCompared.alloc((size_t)idmEntries) || dIdentity.alloc((size_t)idmEntries))
                        return fail(me + ": out of device memory");
                HIPCHK(hipMemcpyAsync(dIdmFirst.p, first.data(), sizeof(int) * first.size(), hipMemcpyHostToDevice, stream));
                HIPCHK(hipMemcpyAsync(dIdmTiles.p, tiles.data(), sizeof(unsigned) * tiles.size(), hipMemcpyHostToDevice, stream));
                KaIdmTab a{};
                a.nFam = nFam; a.nTiles = (int)tiles.size(); a.gap = gap;
                a.fams = dFams.p; a.tileFirst = dIdmFirst.p; a.entFirst = dIdmFirst.p + nFam + 1; a.tiles = dIdmTiles.p; a.rows = dRows.p; a.bytes = bytes;
                a.matches = dMatches.p; a.compared = dCompared.p; a.identity = dIdentity.p;
                HIPCHK(hipEventRecord(ev[0], stream));
                if (ka_sum_run_identity(a, stream, &launches)) return fail(me + ": the identity kernel's LDS was refused");
                HIPCHK(hipGetLastError());
                HIPCHK(hipEventRecord(ev[1], stream));
        }
        const size_t n = (size_t)idmEntries;
        if (matchesOut) HIPCHK(hipMemcpyAsync(matchesOut, dMatches.p, sizeof(int) * n, hipMemcpyDeviceToHost, stream));
        if (comparedOut) HIPCHK(hipMemcpyAsync(comparedOut, dCompared.p, sizeof(int) * n, hipMemcpyDeviceToHost, stream));
        if (identityOut) HIPCHK(hipMemcpyAsync(identityOut, dIdentity.p, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (compute) {
                idmSt[0] = ms(); idmSt[1] = launches; idmSt[2] = 1;
                haveIdm = true;
        }
        return KA_OK;
}

extern "C" long long ka_sum_fam_identity_entries(int n_fam, const int* fam_first)
{
        return idm_entries("ka_sum_fam_identity_entries", n_fam, fam_first);
}

extern "C" int ka_sum_fam_identity(ka_sum_fam* h, int* matches_out, int* compared_out, double* identity_out)
{
        if (!h) return fail("ka_sum_fam_identity: bad arguments");
        return h->identity("ka_sum_fam_identity", matches_out, compared_out, identity_out);
}

extern "C" int ka_sum_fam_identity_stats(ka_sum_fam* h, double* out3)
{
        if (!h) return fail("ka_sum_fam_identity_stats: bad arguments");
        if (out3) std::copy_n(h->idmSt, KA_SUM_IDM_STATS, out3);
        return KA_OK;
}

long long ka_sum_fam::characters() const
{
        long long n = 0;
        for (int f = 0; f < nFam; f++) n += (long long)fams[f].N * fams[f].W - (long long)famSums[(size_t)f * KA_SUM_FAMSUMS + KA_SUM_GAPS];
        return n;
}

// The first-row table up, the row pass and the gappy pass over the whole batch, the records and the sums down, one wait.
// They stay on the host: every later call is a copy from there.
int ka_sum_fam::gaps(const char* who)
{
        if (haveGaps) return KA_OK;
        const std::string me(who);
        int launches = 0;
        HIPCHK(hipSetDevice(device));
        rowFirst.assign((size_t)nFam + 1, 0);
        for (int f = 0; f < nFam; f++) rowFirst[f + 1] = rowFirst[f] + fams[f].N;
        gapRecs.assign((size_t)numseq * KA_SUM_ROWREC, 0);
        gapSums.assign((size_t)nFam * KA_SUM_GAPSUMS, 0);
        if (dRowFirst.alloc(rowFirst.size()) || dGapRecs.alloc(gapRecs.size()) || dGapSums.alloc(gapSums.size())) return fail(me + ": out of device memory");
        HIPCHK(hipMemcpyAsync(dRowFirst.p, rowFirst.data(), sizeof(int) * rowFirst.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemsetAsync(dGapSums.p, 0, sizeof(unsigned long long) * gapSums.size(), stream));
        HIPCHK(hipEventRecord(ev[0], stream));
        ka_sum_run_gaps(gapTab(), stream, &launches);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], stream));
        HIPCHK(hipMemcpyAsync(gapRecs.data(), dGapRecs.p, sizeof(int) * gapRecs.size(), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(gapSums.data(), dGapSums.p, sizeof(unsigned long long) * gapSums.size(), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        gapSt[0] = ms(); gapSt[2] = launches; gapSt[3] = 1;
        haveGaps = true;
        return KA_OK;
}

// Where every row's characters start, a running sum of the records' characters on the host, goes up in one copy; one launch
// packs the rows.  A batch without a character launches nothing.  The rows stay on the device: later calls copy.
int ka_sum_fam::ungapped(const char* who, uint8_t* out, long long cap, long long* rowOffOut)
{
        const std::string me(who);
        const long long size = characters();
        if (cap < size) return fail(me + ": " + std::to_string(cap) + " bytes do not hold the ungapped rows (" + std::to_string(size) + ")");
        if (!out && size > 0) return fail(me + ": bad arguments");
        if (gaps(who)) return KA_FAIL;
        HIPCHK(hipSetDevice(device));
        const bool compute = !haveUngap;
        int launches = 0;
        if (compute) {
                ungapOff.assign((size_t)numseq + 1, 0);
                for (int r = 0; r < numseq; r++) ungapOff[r + 1] = ungapOff[r] + gapRecs[(size_t)r * KA_SUM_ROWREC + KA_ROW_CHARS];
                if (ungapOff[numseq] != size)
                        return fail(me + ": the rows hold " + std::to_string(ungapOff[numseq]) + " characters, the column table " + std::to_string(size));
                if (size > 0) {
                        if (dUngapOff.alloc(ungapOff.size()) || dUngap.alloc((size_t)size)) return fail(me + ": out of device memory");
                        HIPCHK(hipMemcpyAsync(dUngapOff.p, ungapOff.data(), sizeof(long long) * ungapOff.size(), hipMemcpyHostToDevice, stream));
                        HIPCHK(hipEventRecord(ev[0], stream));
                        ka_sum_run_ungap(gapTab(), stream, &launches);
                        HIPCHK(hipGetLastError());
                        HIPCHK(hipEventRecord(ev[1], stream));
                }
        }
        if (size > 0) {
                HIPCHK(hipMemcpyAsync(out, dUngap.p, (size_t)size, hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
        }
        if (compute) {
                if (size > 0) { gapSt[1] = ms(); gapSt[4] = launches; gapSt[5] = 1; }
                haveUngap = true;
        }
        if (rowOffOut) std::copy(ungapOff.begin(), ungapOff.end(), rowOffOut);
        return KA_OK;
}

extern "C" int ka_sum_fam_gap_values(int n_fam, const long long* counts, double* values_out)
{
        if (n_fam < 1 || !counts || !values_out) return fail("ka_sum_fam_gap_values: bad arguments");
        for (int f = 0; f < n_fam; f++) gap_finish(counts + (size_t)f * KA_SUM_GAP_COUNTS, values_out + (size_t)f * KA_SUM_GAP_VALUES);
        return KA_OK;
}

extern "C" int ka_sum_fam_gaps(ka_sum_fam* h, long long* counts_out, double* values_out, int* row_recs_out)
{
        if (!h) return fail("ka_sum_fam_gaps: bad arguments");
        if (h->gaps("ka_sum_fam_gaps")) return KA_FAIL;
        for (int f = 0; f < h->nFam; f++) {
                const unsigned long long* s = &h->gapSums[(size_t)f * KA_SUM_GAPSUMS];
                const KaSumFam& d = h->fams[f];
                const long long cells = (long long)d.N * d.W;
                const long long counts[KA_SUM_GAP_COUNTS] = { d.N, d.W, (long long)s[KA_GAP_CHARS], cells - (long long)s[KA_GAP_CHARS], (long long)s[KA_GAP_BLOCKS],
                                                              (long long)s[KA_GAP_TERMINAL], (long long)s[KA_GAP_INTERNAL], (long long)s[KA_GAP_GAPPY] };
                if (counts_out) std::copy_n(counts, KA_SUM_GAP_COUNTS, counts_out + (size_t)f * KA_SUM_GAP_COUNTS);
                if (values_out) gap_finish(counts, values_out + (size_t)f * KA_SUM_GAP_VALUES);
        }
        if (row_recs_out) std::copy(h->gapRecs.begin(), h->gapRecs.end(), row_recs_out);
        return KA_OK;
}

extern "C" long long ka_sum_fam_ungapped_size(ka_sum_fam* h)
{
        if (!h) return fail("ka_sum_fam_ungapped_size: bad arguments"), -1;
        return h->characters();
}

extern "C" int ka_sum_fam_ungapped(ka_sum_fam* h, uint8_t* out, long long cap, long long* row_off_out)
{
        if (!h) return fail("ka_sum_fam_ungapped: bad arguments");
        return h->ungapped("ka_sum_fam_ungapped", out, cap, row_off_out);
}

extern "C" int ka_sum_fam_gap_stats(ka_sum_fam* h, double* out6)
{
        if (!h) return fail("ka_sum_fam_gap_stats: bad arguments");
        if (out6) std::copy_n(h->gapSt, KA_SUM_GAP_STATS, out6);
        return KA_OK;
}

extern "C" int ka_sum_fam_stats(ka_sum_fam* h, double* stats_out)
{
        if (!h) return fail("ka_sum_fam_stats: bad arguments");
        h->st[4] = h->nLaunch; h->st[5] = h->nSync;
        if (stats_out) std::copy_n(h->st, KA_SUM_STATS, stats_out);
        return KA_OK;
}
