// ka_cmp.cpp -- host side of scoring alignments against reference alignments (kalign_msa_compare*, lib/src/msa_cmp.c):
// the core both handles of the C ABI stand on, and the ka_cmp handle (K test alignments of one reference).  The ka_cmp_fam
// handle (a batch of families, one test each) is ka_cmp_fam.cpp.
//
// The core holds the references of a handle -- their position maps, per-column residue counts and scored columns, built
// once -- and scores a call's jobs (ka_cmp.h: one test alignment against one reference) in one sequence: the rows
// uploaded, the test maps, the pair walk (one launch per LDS class in use), the TC pass, every job's eight sums back in
// one copy behind one synchronisation (ka_cmp.hip).  The device returns exact integer counts; the final doubles are
// computed on the host with the reference's expressions, in its order (ka_cmp_finish, ka_cmp.h).  A detail call (one
// job per reference) takes the same first steps -- begin() and walk() are shared -- with the walk in its detailed form,
// then the column pass, and brings the counts of every residue and the records of every column back in one copy.
//
// A handle's front checks its arguments on the host before anything is launched and says how its rows are laid out; a
// refused call launches nothing and leaves the handle usable.
//
// Unlike the reference, the two alignments must hold the same sequences: numseq rows each, row s with lens[s] letters
// (the reference reads out of bounds otherwise).  Two sequences at least.
#include "ka_cmp_core.h"

#include <string.h>

namespace {

constexpr int kGroup = 32;         // test alignments per device pass of ka_cmp_score_batch: the bound on device memory

// the LDS the walk needs for a job: TJ rows of both maps, as many as the budget holds, one at least; *tj = 0 when one row
// pair does not fit a CU
size_t walk_lds(int N, int WRp, int WTp, int* tj)
{
        const size_t rowBytes = (size_t)(WRp + WTp) * sizeof(int16_t);
        int TJ = (int)std::min<size_t>(KA_CMP_TJ, KA_CMP_LDS / rowBytes);
        TJ = std::max(1, std::min(TJ, N));
        const size_t lds = (size_t)TJ * rowBytes;
        *tj = lds > KA_CMP_MAX_LDS - 1024 ? 0 : TJ;
        return lds;
}

int lds_class(size_t lds)
{
        int c = 0;
        while (c < KA_CMP_CLASSES - 1 && lds > ((size_t)KA_CMP_LDS >> (KA_CMP_CLASSES - 2 - c))) c++;
        return c;
}

// "<who>" or "<who>: <item> <k>"
std::string at(const char* who, const char* item, int k)
{
        return item ? std::string(who) + ": " + item + " " + std::to_string(k) : std::string(who);
}

} // namespace

KaCmpCore::~KaCmpCore()
{
        for (auto& e : ev)
                if (e) (void)hipEventDestroy(e);
}

int KaCmpCore::attach(ka_ctx* ctx) { return ka_ctx_device_stream(ctx, &device, &stream); }

void KaCmpCore::close()
{
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
}

KaCmpTab KaCmpCore::tab() const
{
        KaCmpTab a{};
        const int nRef = (int)refs.size();
        a.nRef = nRef; a.S = S; a.cols = cols;
        a.refs = dRefs.p; a.refSeq = dRefFirst.p; a.refCol = dRefFirst.p + nRef + 1;
        a.offs = dOffs.p; a.lens = dLens.p; a.seqOf = dSeqOf.p; a.rows = dRows.p;
        a.colR = dColR.p; a.colT = dColT.p; a.resR = dResR.p; a.resT = dResT.p;
        a.colCnt = dColCnt.p; a.scored = dScored.p; a.sums = dSums.p;
        return a;
}

int KaCmpCore::create(const char* who, const char* item, int nRef, const int* first, const int* l, const int* widths, int pad, const KaCmpUpload& upload)
{
        const std::string me(who);
        S = first[nRef];
        lens.assign(l, l + S);
        offs.resize(S + 1);
        int t = 0;
        for (int s = 0; s < S; s++) { offs[s] = t; t += l[s]; }
        offs[S] = T = t;
        refs.assign(nRef, KaCmpJob{});
        std::vector<int> refFirst((size_t)2 * (nRef + 1)), seqOf((size_t)std::max(T, 1), 0);
        long long rowOff = 0, resOff = 0;
        int col = 0;
        for (int f = 0; f < nRef; f++) {
                KaCmpJob& d = refs[f];
                d.firstSeq = first[f]; d.firstRes = offs[first[f]]; d.firstCol = col;
                d.N = first[f + 1] - first[f];
                d.r.W = widths[f]; d.r.Wp = ka_cmp_pad(widths[f]); d.r.stride = widths[f] + pad; d.r.rowOff = rowOff; d.r.resOff = resOff;
                if ((size_t)d.r.Wp * 2 * sizeof(int16_t) > KA_CMP_MAX_LDS - 1024)
                        return fail(at(who, item, f) + ": reference width " + std::to_string(d.r.W) +
                                    " exceeds the LDS of one CU (a row of each alignment is staged)");
                for (int s = 0; s < d.N; s++) std::fill_n(seqOf.begin() + offs[d.firstSeq + s], l[d.firstSeq + s], s);
                refFirst[f] = first[f];
                refFirst[nRef + 1 + f] = col;
                col += d.r.W;
                rowOff += d.N * d.r.stride;
                resOff += (long long)d.N * d.r.Wp;
        }
        refFirst[nRef] = S;
        refFirst[2 * nRef + 1] = cols = col;
        HIPCHK(hipSetDevice(device));
        for (auto& e : ev) HIPCHK(hipEventCreate(&e));
        if (dRefs.alloc(nRef) || dRefFirst.alloc(refFirst.size()) || dOffs.alloc(S + 1) || dLens.alloc(S) || dSeqOf.alloc(seqOf.size()) ||
            dColR.alloc(seqOf.size()) || dResR.alloc((size_t)resOff) || dColCnt.alloc(col) || dScored.alloc(col) || dRows.alloc((size_t)rowOff) ||
            dFrac.alloc(nRef) || dMaskOff.alloc(nRef))
                return fail(me + ": out of device memory");
        HIPCHK(hipMemcpyAsync(dRefs.p, refs.data(), sizeof(KaCmpJob) * nRef, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dRefFirst.p, refFirst.data(), sizeof(int) * refFirst.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dOffs.p, offs.data(), sizeof(int) * (S + 1), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dLens.p, lens.data(), sizeof(int) * S, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dSeqOf.p, seqOf.data(), sizeof(int) * seqOf.size(), hipMemcpyHostToDevice, stream));
        if (upload(dRows.p, stream)) return KA_FAIL;
        HIPCHK(hipEventRecord(ev[0], stream));
        const KaCmpTab a = tab();                                // (no fractions, no masks: every column is scored)
        ka_cmp_run_maps(a, 0, stream);
        ka_cmp_run_col_count(a, stream);
        ka_cmp_run_mask(a, stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], stream));
        HIPCHK(hipStreamSynchronize(stream));                    // (refFirst and seqOf are read until here)
        st[0] = ms(0, 1);
        return KA_OK;
}

int KaCmpCore::set_rule(const char* who, const float* frac, const int* masks, const long long* maskOff, long long nMask)
{
        const int nRef = (int)refs.size();
        HIPCHK(hipSetDevice(device));
        if (nMask && dMasks.alloc((size_t)nMask)) return fail(std::string(who) + ": out of device memory");
        if (nMask) HIPCHK(hipMemcpyAsync(dMasks.p, masks, sizeof(int) * (size_t)nMask, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dFrac.p, frac, sizeof(float) * nRef, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dMaskOff.p, maskOff, sizeof(long long) * nRef, hipMemcpyHostToDevice, stream));
        KaCmpTab a = tab();
        a.frac = dFrac.p; a.masks = dMasks.p; a.maskOff = dMaskOff.p;
        ka_cmp_run_mask(a, stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));                    // (the caller's arrays are read until here)
        return KA_OK;
}

int KaCmpCore::begin(const char* who, const char* item, int nJob, const int* refOf, const int* widths, int pad, const KaCmpUpload& upload, Call& c,
                     int* launches)
{
        const std::string me(who);
        // every job's test side, tile geometry and LDS class, and the ascending tables of what the call numbers: test
        // rows, job columns, test columns and the tiles of every LDS class
        static const char* const what[4] = { "rows", "columns", "test columns", "tiles" };
        c.nJob = nJob;
        c.jobs.assign(nJob, KaCmpJob{});
        c.first.assign((size_t)TABLES * (nJob + 1), 0);
        std::vector<int>& first = c.first;
        long long rowOff = 0, resOff = 0, colOff = 0;
        for (int k = 0; k < nJob; k++) {
                KaCmpJob& d = c.jobs[k] = refs[refOf ? refOf[k] : k];
                d.t.W = widths[k]; d.t.Wp = ka_cmp_pad(widths[k]); d.t.stride = widths[k] + pad; d.t.rowOff = rowOff; d.t.resOff = resOff;
                d.colOff = colOff - d.firstRes;
                const size_t lds = walk_lds(d.N, d.r.Wp, d.t.Wp, &d.TJ);
                if (!d.TJ)
                        return fail(at(who, item, k) + ": reference width " + std::to_string(d.r.W) + " and test width " + std::to_string(d.t.Wp) +
                                    " together exceed the LDS of one CU (one row of each is staged)");
                d.nTJ = (d.N + d.TJ - 1) / d.TJ;
                const int nTI = (d.N + KA_CMP_TI - 1) / KA_CMP_TI, cls = lds_class(lds);
                c.classLds[cls] = std::max(c.classLds[cls], lds);
                for (int t = 0; t < TABLES; t++) {
                        const long long n = t == ROWS ? d.N : t == COLS ? d.r.W : t == TCOLS ? d.t.W : t - TILES == cls ? (long long)nTI * d.nTJ : 0;
                        const long long next = first[(size_t)t * (nJob + 1) + k] + n;
                        if (next > INT32_MAX) return fail(me + ": more than 2^31 - 1 " + what[std::min<int>(t, TILES)] + " in the batch");
                        first[(size_t)t * (nJob + 1) + k + 1] = (int)next;
                }
                rowOff += d.N * d.t.stride;
                resOff += (long long)d.N * d.t.Wp;
                colOff += offs[d.firstSeq + d.N] - d.firstRes;
        }
        HIPCHK(hipSetDevice(device));
        if (dRows.alloc((size_t)rowOff) || dResT.alloc((size_t)resOff) || dColT.alloc((size_t)std::max<long long>(colOff, 1)) || dJobs.alloc(nJob) ||
            dJobFirst.alloc(first.size()) || dSums.alloc((size_t)nJob * KA_CMP_SUMS))
                return fail(me + ": out of device memory");
        HIPCHK(hipMemcpyAsync(dJobs.p, c.jobs.data(), sizeof(KaCmpJob) * nJob, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dJobFirst.p, first.data(), sizeof(int) * first.size(), hipMemcpyHostToDevice, stream));
        if (upload(dRows.p, stream)) return KA_FAIL;
        HIPCHK(hipMemsetAsync(dSums.p, 0, sizeof(unsigned long long) * (size_t)nJob * KA_CMP_SUMS, stream));
        HIPCHK(hipEventRecord(ev[0], stream));
        KaCmpTab& a = c.a = tab();
        a.nJob = nJob; a.jobs = dJobs.p;
        a.jobRow = dJobFirst.p + (size_t)ROWS * (nJob + 1); a.jobRows = c.last(ROWS);
        a.jobCol = dJobFirst.p + (size_t)COLS * (nJob + 1); a.jobCols = c.last(COLS);
        a.tcolFirst = dJobFirst.p + (size_t)TCOLS * (nJob + 1); a.tCols = c.last(TCOLS);
        ka_cmp_run_maps(a, 1, stream);
        ++*launches;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], stream));
        return KA_OK;
}

int KaCmpCore::walk(const char* who, const Call& c, bool detailed, int* launches)
{
        for (int cls = 0; cls < KA_CMP_CLASSES; cls++) {
                const size_t at0 = (size_t)(TILES + cls) * (c.nJob + 1);
                if (!c.last(TILES + cls)) continue;
                if (ka_cmp_run_walk(c.a, dJobFirst.p + at0, c.last(TILES + cls), c.classLds[cls], detailed, stream))
                        return fail(std::string(who) + ": the walk's LDS (" + std::to_string(c.classLds[cls]) + " bytes) was refused");
                ++*launches;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[2], stream));
        return KA_OK;
}

int KaCmpCore::score(const char* who, const char* item, int nJob, const int* refOf, const int* widths, int pad, const KaCmpUpload& upload,
                     long long* counts, double* scores, float* sp)
{
        Call c;
        int launches = 0;
        if (begin(who, item, nJob, refOf, widths, pad, upload, c, &launches) || walk(who, c, false, &launches)) return KA_FAIL;
        std::vector<unsigned long long> sums((size_t)nJob * KA_CMP_SUMS);
        ka_cmp_run_tc(c.a, stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[3], stream));
        HIPCHK(hipMemcpyAsync(sums.data(), dSums.p, sizeof(unsigned long long) * sums.size(), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        st[1] += ms(0, 1); st[2] += ms(1, 2); st[3] += ms(2, 3);
        for (int k = 0; k < nJob; k++) {
                const KaCmpJob& d = c.jobs[k];
                const long long* w = (const long long*)&sums[(size_t)k * KA_CMP_SUMS];
                ka_cmp_finish(w, w[KA_CMP_WALK], w[KA_CMP_WALK + 1], d.N, offs[d.firstSeq + d.N] - d.firstRes,
                              counts ? counts + (size_t)k * 12 : nullptr, scores ? scores + (size_t)k * 5 : nullptr, sp ? sp + k : nullptr);
        }
        return KA_OK;
}

// A detail call's outputs are one block on the device and come back in one copy: the column records' 64-bit sums first
// (8-byte aligned), then the three residue planes (the part the walk adds to: zeroed), the columns' residues and flags
int KaCmpCore::detail(const char* who, const char* item, const int* widths, int pad, const KaCmpUpload& upload, int* resCounts, int* tcolRes,
                      long long* tcolCommon, uint8_t* tcolCorrect, int* rcolRes, long long* rcolCommon, uint8_t* rcolCorrect)
{
        Call c;
        int launches = 0;
        if (begin(who, item, (int)refs.size(), nullptr, widths, pad, upload, c, &launches)) return KA_FAIL;
        const size_t nCol = (size_t)c.a.tCols + (size_t)cols, nT = (size_t)T;
        const size_t oPlanes = nCol * sizeof(long long), oRes = oPlanes + 3 * nT * sizeof(int), oFlag = oRes + nCol * sizeof(int), bytes = oFlag + nCol;
        if (dDet.alloc(bytes)) return fail(std::string(who) + ": out of device memory");
        HIPCHK(hipMemsetAsync(dDet.p + oPlanes, 0, 3 * nT * sizeof(int), stream));
        c.a.T = T;
        c.a.detColCommon = (long long*)dDet.p;
        c.a.detRes = (int*)(dDet.p + oPlanes);
        c.a.detColRes = (int*)(dDet.p + oRes);
        c.a.detColCorrect = dDet.p + oFlag;
        if (walk(who, c, true, &launches)) return KA_FAIL;
        ka_cmp_run_cols(c.a, stream);
        launches += nCol > 0;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[3], stream));
        std::vector<uint8_t> out(bytes);
        HIPCHK(hipMemcpyAsync(out.data(), dDet.p, bytes, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        dst[0] = ms(0, 1); dst[1] = ms(1, 2); dst[2] = ms(2, 3); dst[3] = launches; dst[4] = 1;
        const size_t nt = (size_t)c.a.tCols, nr = (size_t)cols;
        if (resCounts) memcpy(resCounts, out.data() + oPlanes, 3 * nT * sizeof(int));
        if (tcolCommon) memcpy(tcolCommon, out.data(), nt * sizeof(long long));
        if (rcolCommon) memcpy(rcolCommon, out.data() + nt * sizeof(long long), nr * sizeof(long long));
        if (tcolRes) memcpy(tcolRes, out.data() + oRes, nt * sizeof(int));
        if (rcolRes) memcpy(rcolRes, out.data() + oRes + nt * sizeof(int), nr * sizeof(int));
        if (tcolCorrect) memcpy(tcolCorrect, out.data() + oFlag, nt);
        if (rcolCorrect) memcpy(rcolCorrect, out.data() + oFlag + nt, nr);
        return KA_OK;
}

// ---- one reference, K tests: rows `row_stride` apart on the host, uploaded back to back ----
struct ka_cmp {
        KaCmpCore core;
        KaSeqSet q;                // (host side only: the row checks and the strided upload)
};

extern "C" int ka_cmp_create(ka_ctx* ctx, int numseq, const int* lens, const uint8_t* ref_rows, long long row_stride, int alnlen, ka_cmp** out)
{
        if (!ctx || !out || !lens) return fail("ka_cmp_create: bad arguments");
        *out = nullptr;
        if (numseq < 2) return fail("ka_cmp_create: " + std::to_string(numseq) + " sequences; a comparison needs two at least");
        std::unique_ptr<ka_cmp> h(new ka_cmp);
        if (h->core.attach(ctx)) return fail("ka_cmp_create: bad context");
        const std::string why = "the position maps hold at most " + std::to_string(KA_CMP_MAX_RES);
        if (h->q.set("ka_cmp_create", numseq, lens, KA_CMP_MAX_RES, why.c_str())) return KA_FAIL;
        if (ka_msa_check_rows("ka_cmp_create", h->q, ref_rows, row_stride, alnlen)) return KA_FAIL;
        const int first[2] = { 0, numseq };
        const KaSeqSet& q = h->q;
        if (h->core.create("ka_cmp_create", nullptr, 1, first, lens, &alnlen, 0, [&](uint8_t* dst, hipStream_t s) {
                    return ka_msa_upload_rows(q, dst, ref_rows, row_stride, alnlen, s);
            }))
                return KA_FAIL;
        *out = h.release();
        return KA_OK;
}

extern "C" void ka_cmp_destroy(ka_cmp* h)
{
        if (!h) return;
        h->core.close();
        delete h;
}

extern "C" int ka_cmp_set_mask(ka_cmp* h, float max_gap_frac, const int* mask, int n_cols)
{
        if (!h) return fail("ka_cmp_set_mask: bad arguments");
        const int WR = h->core.refs[0].r.W;
        if (mask && n_cols != WR)
                return fail("ka_cmp_set_mask: mask length " + std::to_string(n_cols) + " != reference alignment length " + std::to_string(WR));
        const long long off = mask ? 0 : -1;
        return h->core.set_rule("ka_cmp_set_mask", &max_gap_frac, mask, &off, mask ? WR : 0);
}

extern "C" int ka_cmp_score_batch(ka_cmp* h, int n_tests, const uint8_t* const* test_rows, const long long* row_strides, const int* alnlens,
                                  long long* counts_out, double* scores_out, float* sp_out)
{
        if (!h || n_tests < 0 || (n_tests > 0 && (!test_rows || !row_strides || !alnlens))) return fail("ka_cmp_score_batch: bad arguments");
        for (int k = 0; k < n_tests; k++) {
                const std::string who = "ka_cmp_score: test " + std::to_string(k);
                if (ka_msa_check_rows(who.c_str(), h->q, test_rows[k], row_strides[k], alnlens[k])) return KA_FAIL;
        }
        std::fill_n(h->core.st + 1, KA_CMP_STATS - 1, 0.0);
        const std::vector<int> refOf(kGroup, 0);
        const KaSeqSet& q = h->q;
        for (int k0 = 0; k0 < n_tests; k0 += kGroup) {
                const int K = std::min(kGroup, n_tests - k0);
                auto upload = [&](uint8_t* dst, hipStream_t s) {
                        for (int k = k0; k < k0 + K; dst += (long long)q.N * alnlens[k], k++)
                                if (ka_msa_upload_rows(q, dst, test_rows[k], row_strides[k], alnlens[k], s)) return (int)KA_FAIL;
                        return (int)KA_OK;
                };
                if (h->core.score("ka_cmp_score", nullptr, K, refOf.data(), alnlens + k0, 0, upload, counts_out ? counts_out + (size_t)k0 * 12 : nullptr,
                                  scores_out ? scores_out + (size_t)k0 * 5 : nullptr, sp_out ? sp_out + k0 : nullptr))
                        return KA_FAIL;
        }
        return KA_OK;
}

extern "C" int ka_cmp_score(ka_cmp* h, const uint8_t* test_rows, long long row_stride, int alnlen, long long* counts_out, double* scores_out, float* sp_out)
{
        return ka_cmp_score_batch(h, 1, &test_rows, &row_stride, &alnlen, counts_out, scores_out, sp_out);
}

extern "C" int ka_cmp_stats(ka_cmp* h, double* stats_out)
{
        if (!h) return fail("ka_cmp_stats: bad arguments");
        if (stats_out) std::copy_n(h->core.st, KA_CMP_STATS, stats_out);
        return KA_OK;
}

extern "C" int ka_cmp_detail(ka_cmp* h, const uint8_t* test_rows, long long row_stride, int alnlen, int* res_counts, int* tcol_residues,
                             long long* tcol_common, uint8_t* tcol_correct, int* rcol_residues, long long* rcol_common, uint8_t* rcol_correct)
{
        if (!h) return fail("ka_cmp_detail: bad arguments");
        std::fill_n(h->core.dst, KA_CMP_DETAIL_STATS, 0.0);
        if (ka_msa_check_rows("ka_cmp_detail", h->q, test_rows, row_stride, alnlen)) return KA_FAIL;
        const KaSeqSet& q = h->q;
        return h->core.detail("ka_cmp_detail", nullptr, &alnlen, 0, [&](uint8_t* dst, hipStream_t s) {
                return ka_msa_upload_rows(q, dst, test_rows, row_stride, alnlen, s);
        }, res_counts, tcol_residues, tcol_common, tcol_correct, rcol_residues, rcol_common, rcol_correct);
}

extern "C" int ka_cmp_detail_stats(ka_cmp* h, double* out5)
{
        if (!h) return fail("ka_cmp_detail_stats: bad arguments");
        if (out5) std::copy_n(h->core.dst, KA_CMP_DETAIL_STATS, out5);
        return KA_OK;
}
