// ka_cmp_fam.cpp -- host side of scoring a batch of families, each against its own reference alignment: the ka_cmp_fam
// handle of the C ABI (ka_cmp.cpp is the one-reference form; the kernels are ka_cmp_fam.hip).
//
// The references' position maps, column counts and the per-family tables are built once (ka_cmp_fam_create); a score
// call uploads the packed test rows in one copy, runs the test maps, the pair walk (one launch per LDS class in use) and
// the TC pass over all families, and brings every family's eight sums back in one copy behind one synchronisation.  The
// doubles come from ka_cmp_finish (ka_cmp.h), the function ka_cmp_score ends in.
//
// Every check runs on the host before anything is launched (cmp_fam_check; ka_cmp_fam_check is its public form), with
// the functions the one-family calls use (KaSeqSet::set, ka_msa_check_rows): a family is refused with the cause it is
// refused with alone.
#include "ka_ctx.h"
#include "ka_cmp.h"
#include "ka_msa.h"

int ka_ctx_device_stream(ka_ctx* c, int* device, hipStream_t* stream);    // (library-internal: ka_api.cpp)

namespace {

// the LDS the walk needs for a family: TJ rows of both maps (ka_cmp::score's rule); 0 with *tj = 0 when one row pair does not fit a CU
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
        while (c < KA_CMPF_CLASSES - 1 && lds > ((size_t)KA_CMP_LDS >> (KA_CMPF_CLASSES - 2 - c))) c++;
        return c;
}

// a packed batch on the host alone: the families, their sequences and their rows
int cmp_fam_check(const char* who, int n_fam, const int* fam_first, const int* lens, const uint8_t* rows, const int* alnlens)
{
        const std::string me(who);
        if (n_fam < 1 || !fam_first || !lens || !rows || !alnlens) return fail(me + ": bad arguments");
        if (fam_first[0] != 0) return fail(me + ": fam_first does not ascend from 0 to numseq");
        for (int f = 0; f < n_fam; f++) {
                if (fam_first[f + 1] < fam_first[f]) return fail(me + ": fam_first does not ascend from 0 to numseq");
                if (fam_first[f + 1] == fam_first[f]) return fail(me + ": empty family");
        }
        const std::string why = "the position maps hold at most " + std::to_string(KA_CMP_MAX_RES);
        long long residues = 0, cols = 0, off = 0;
        for (int f = 0; f < n_fam; f++) {
                const std::string fam = me + ": family " + std::to_string(f);
                const int N = fam_first[f + 1] - fam_first[f];
                if (N < 2) return fail(fam + ": " + std::to_string(N) + " sequences; a comparison needs two at least");
                KaSeqSet q;                                      // (host side only: nothing to release)
                if (q.set(fam.c_str(), N, lens + fam_first[f], KA_CMP_MAX_RES, why.c_str())) return KA_FAIL;
                if (ka_msa_check_rows(fam.c_str(), q, rows + off, (long long)alnlens[f] + 1, alnlens[f])) return KA_FAIL;
                residues += q.T;
                cols += alnlens[f];
                off += (long long)N * (alnlens[f] + 1);
                if (residues > INT32_MAX) return fail(me + ": more than 2^31 - 1 residues in the batch");
                if (cols > INT32_MAX) return fail(me + ": more than 2^31 - 1 columns in the batch");
        }
        return KA_OK;
}

} // namespace

struct ka_cmp_fam {
        int device = 0;
        hipStream_t stream = nullptr;
        int nFam = 0, S = 0, T = 0, cols = 0;
        std::vector<int> famFirst, lens, offs, firstCol;
        std::vector<KaCmpFam> fams;                              // the reference side filled by create, the test side by score
        std::vector<int> tileFirst;                              // [KA_CMPF_CLASSES][nFam + 1]
        std::vector<unsigned long long> sums;
        DevBuf<KaCmpFam> dFams;
        DevBuf<int> dFirstSeq, dFirstCol, dOffs, dLens, dSeqOf, dColR, dColT, dColCnt, dMasks, dTileFirst;
        DevBuf<int16_t> dResR, dResT;
        DevBuf<uint8_t> dRows, dScored;
        DevBuf<float> dFrac;
        DevBuf<long long> dMaskOff;
        DevBuf<unsigned long long> dSums;
        hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
        double st[KA_CMP_STATS] = {};

        ~ka_cmp_fam()
        {
                for (auto& e : ev)
                        if (e) (void)hipEventDestroy(e);
                dFams.release(); dFirstSeq.release(); dFirstCol.release(); dOffs.release(); dLens.release(); dSeqOf.release();
                dColR.release(); dColT.release(); dColCnt.release(); dMasks.release(); dTileFirst.release(); dResR.release();
                dResT.release(); dRows.release(); dScored.release(); dFrac.release(); dMaskOff.release(); dSums.release();
        }

        float ms(int a, int b) { float m = 0.0f; (void)hipEventElapsedTime(&m, ev[a], ev[b]); return m; }

        KaCmpFamArgs args() const
        {
                KaCmpFamArgs a{};
                a.nFam = nFam; a.S = S; a.cols = cols;
                a.fams = dFams.p; a.firstSeq = dFirstSeq.p; a.firstCol = dFirstCol.p; a.offs = dOffs.p; a.lens = dLens.p; a.seqOf = dSeqOf.p;
                a.rows = dRows.p; a.colR = dColR.p; a.colT = dColT.p; a.resR = dResR.p; a.resT = dResT.p;
                a.colCnt = dColCnt.p; a.scored = dScored.p; a.sums = dSums.p;
                return a;
        }
};

extern "C" int ka_cmp_fam_check(int n_fam, const int* fam_first, const int* lens, const uint8_t* rows, const int* alnlens)
{
        return cmp_fam_check("ka_cmp_fam_check", n_fam, fam_first, lens, rows, alnlens);
}

extern "C" int ka_cmp_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const int* lens, const uint8_t* ref_rows, const int* ref_alnlens,
                                 ka_cmp_fam** out)
{
        if (!ctx || !out) return fail("ka_cmp_fam_create: bad arguments");
        *out = nullptr;
        if (cmp_fam_check("ka_cmp_fam_create", n_fam, fam_first, lens, ref_rows, ref_alnlens)) return KA_FAIL;
        std::unique_ptr<ka_cmp_fam> h(new ka_cmp_fam);
        if (ka_ctx_device_stream(ctx, &h->device, &h->stream)) return fail("ka_cmp_fam_create: bad context");
        const int S = fam_first[n_fam];
        h->nFam = n_fam; h->S = S;
        h->famFirst.assign(fam_first, fam_first + n_fam + 1);
        h->lens.assign(lens, lens + S);
        h->offs.resize(S + 1);
        h->firstCol.resize(n_fam + 1);
        h->fams.resize(n_fam);
        h->tileFirst.resize((size_t)KA_CMPF_CLASSES * (n_fam + 1));
        h->sums.resize((size_t)n_fam * KA_CMPF_SUMS);
        int t = 0;
        for (int s = 0; s < S; s++) { h->offs[s] = t; t += lens[s]; }
        h->offs[S] = h->T = t;
        std::vector<int> seqOf((size_t)std::max(t, 1), 0);
        long long rowOff = 0, resOff = 0;
        int col = 0;
        for (int f = 0; f < n_fam; f++) {
                KaCmpFam& d = h->fams[f];
                d = KaCmpFam{};
                d.firstSeq = fam_first[f]; d.firstRes = h->offs[fam_first[f]]; d.firstCol = col;
                d.N = fam_first[f + 1] - fam_first[f];
                d.r.W = ref_alnlens[f]; d.r.Wp = ka_cmp_pad(ref_alnlens[f]); d.r.rowOff = rowOff; d.r.resOff = resOff;
                if ((size_t)d.r.Wp * 2 * sizeof(int16_t) > KA_CMP_MAX_LDS - 1024)
                        return fail("ka_cmp_fam_create: family " + std::to_string(f) + ": reference width " + std::to_string(d.r.W) +
                                    " exceeds the LDS of one CU (a row of each alignment is staged)");
                for (int s = 0; s < d.N; s++) std::fill_n(seqOf.begin() + h->offs[d.firstSeq + s], lens[d.firstSeq + s], s);
                h->firstCol[f] = col;
                col += d.r.W;
                rowOff += (long long)d.N * (d.r.W + 1);
                resOff += (long long)d.N * d.r.Wp;
        }
        h->firstCol[n_fam] = h->cols = col;
        HIPCHK(hipSetDevice(h->device));
        for (auto& e : h->ev) HIPCHK(hipEventCreate(&e));
        if (h->dFams.alloc(n_fam) || h->dFirstSeq.alloc(n_fam + 1) || h->dFirstCol.alloc(n_fam + 1) || h->dOffs.alloc(S + 1) || h->dLens.alloc(S) ||
            h->dSeqOf.alloc(seqOf.size()) || h->dColR.alloc(seqOf.size()) || h->dColT.alloc(seqOf.size()) || h->dResR.alloc((size_t)resOff) ||
            h->dColCnt.alloc(col) || h->dScored.alloc(col) || h->dRows.alloc((size_t)rowOff) || h->dFrac.alloc(n_fam) || h->dMaskOff.alloc(n_fam) ||
            h->dTileFirst.alloc(h->tileFirst.size()) || h->dSums.alloc(h->sums.size()))
                return fail("ka_cmp_fam_create: out of device memory");
        hipStream_t st = h->stream;
        HIPCHK(hipMemcpyAsync(h->dFams.p, h->fams.data(), sizeof(KaCmpFam) * n_fam, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dFirstSeq.p, h->famFirst.data(), sizeof(int) * (n_fam + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dFirstCol.p, h->firstCol.data(), sizeof(int) * (n_fam + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dOffs.p, h->offs.data(), sizeof(int) * (S + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dLens.p, h->lens.data(), sizeof(int) * S, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dSeqOf.p, seqOf.data(), sizeof(int) * seqOf.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dRows.p, ref_rows, (size_t)rowOff, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(h->ev[0], st));
        KaCmpFamArgs a = h->args();                              // (no fractions, no masks: every column is scored)
        ka_cmpf_launch_maps(a, 0, st);
        ka_cmpf_launch_col_count(a, st);
        ka_cmpf_launch_mask(a, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev[1], st));
        HIPCHK(hipStreamSynchronize(st));
        h->st[0] = h->ms(0, 1);
        *out = h.release();
        return KA_OK;
}

extern "C" void ka_cmp_fam_destroy(ka_cmp_fam* h)
{
        if (!h) return;
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        delete h;
}

extern "C" int ka_cmp_fam_set_masks(ka_cmp_fam* h, const float* max_gap_frac, const int* masks, const long long* mask_off)
{
        if (!h) return fail("ka_cmp_fam_set_masks: bad arguments");
        const int F = h->nFam;
        std::vector<float> frac(F, -1.0f);
        std::vector<long long> off(F, -1);
        if (max_gap_frac) std::copy_n(max_gap_frac, F, frac.begin());
        long long n = 0;                                         // ints of `masks` in use
        if (masks && mask_off)
                for (int f = 0; f < F; f++) {
                        if (mask_off[f] < 0) continue;
                        off[f] = mask_off[f];
                        n = std::max(n, mask_off[f] + h->fams[f].r.W);
                }
        HIPCHK(hipSetDevice(h->device));
        if (n && h->dMasks.alloc((size_t)n)) return fail("ka_cmp_fam_set_masks: out of device memory");
        if (n) HIPCHK(hipMemcpyAsync(h->dMasks.p, masks, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->dFrac.p, frac.data(), sizeof(float) * F, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->dMaskOff.p, off.data(), sizeof(long long) * F, hipMemcpyHostToDevice, h->stream));
        KaCmpFamArgs a = h->args();
        a.frac = h->dFrac.p; a.masks = h->dMasks.p; a.maskOff = h->dMaskOff.p;
        ka_cmpf_launch_mask(a, h->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));                 // (frac and off are read until here)
        return KA_OK;
}

extern "C" int ka_cmp_fam_score(ka_cmp_fam* h, const uint8_t* test_rows, const int* test_alnlens, long long* counts_out, double* scores_out,
                                float* sp_out)
{
        if (!h) return fail("ka_cmp_fam_score: bad arguments");
        const int F = h->nFam;
        if (cmp_fam_check("ka_cmp_fam_score", F, h->famFirst.data(), h->lens.data(), test_rows, test_alnlens)) return KA_FAIL;
        // the test side of every family, its tile geometry and its LDS class -- on a copy: a refused batch leaves the handle as it was
        std::vector<KaCmpFam> fams = h->fams;
        std::vector<int> tileFirst((size_t)KA_CMPF_CLASSES * (F + 1), 0);
        size_t classLds[KA_CMPF_CLASSES] = {};
        long long rowOff = 0, resOff = 0;
        for (int f = 0; f < F; f++) {
                KaCmpFam& d = fams[f];
                d.t.W = test_alnlens[f]; d.t.Wp = ka_cmp_pad(test_alnlens[f]); d.t.rowOff = rowOff; d.t.resOff = resOff;
                const size_t lds = walk_lds(d.N, d.r.Wp, d.t.Wp, &d.TJ);
                if (!d.TJ)
                        return fail("ka_cmp_fam_score: family " + std::to_string(f) + ": reference width " + std::to_string(d.r.W) + " and test width " +
                                    std::to_string(d.t.Wp) + " together exceed the LDS of one CU (one row of each is staged)");
                d.nTJ = (d.N + d.TJ - 1) / d.TJ;
                const int nTI = (d.N + KA_CMP_TI - 1) / KA_CMP_TI, cls = lds_class(lds);
                classLds[cls] = std::max(classLds[cls], lds);
                for (int c = 0; c < KA_CMPF_CLASSES; c++) {
                        const long long next = (long long)tileFirst[(size_t)c * (F + 1) + f] + (c == cls ? (long long)nTI * d.nTJ : 0);
                        if (next > INT32_MAX) return fail("ka_cmp_fam_score: more than 2^31 - 1 tiles in the batch");
                        tileFirst[(size_t)c * (F + 1) + f + 1] = (int)next;
                }
                rowOff += (long long)d.N * (d.t.W + 1);
                resOff += (long long)d.N * d.t.Wp;
        }
        HIPCHK(hipSetDevice(h->device));
        if (h->dRows.alloc((size_t)rowOff) || h->dResT.alloc((size_t)resOff)) return fail("ka_cmp_fam_score: out of device memory");
        h->fams.swap(fams);
        h->tileFirst.swap(tileFirst);
        hipStream_t st = h->stream;
        HIPCHK(hipMemcpyAsync(h->dFams.p, h->fams.data(), sizeof(KaCmpFam) * F, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dTileFirst.p, h->tileFirst.data(), sizeof(int) * h->tileFirst.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dRows.p, test_rows, (size_t)rowOff, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(h->dSums.p, 0, sizeof(unsigned long long) * h->sums.size(), st));
        HIPCHK(hipEventRecord(h->ev[0], st));
        KaCmpFamArgs a = h->args();
        ka_cmpf_launch_maps(a, 1, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev[1], st));
        for (int c = 0; c < KA_CMPF_CLASSES; c++) {
                const int nTiles = h->tileFirst[(size_t)c * (F + 1) + F];
                if (!nTiles) continue;
                if (ka_cmpf_launch_walk(a, h->dTileFirst.p + (size_t)c * (F + 1), nTiles, classLds[c], st))
                        return fail("ka_cmp_fam_score: the walk's LDS (" + std::to_string(classLds[c]) + " bytes) was refused");
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev[2], st));
        ka_cmpf_launch_tc(a, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev[3], st));
        HIPCHK(hipMemcpyAsync(h->sums.data(), h->dSums.p, sizeof(unsigned long long) * h->sums.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        h->st[1] = h->ms(0, 1); h->st[2] = h->ms(1, 2); h->st[3] = h->ms(2, 3);
        for (int f = 0; f < F; f++) {
                const KaCmpFam& d = h->fams[f];
                const long long* w = (const long long*)&h->sums[(size_t)f * KA_CMPF_SUMS];
                ka_cmp_finish(w, w[KA_CMP_WALK], w[KA_CMP_WALK + 1], d.N, h->offs[d.firstSeq + d.N] - d.firstRes,
                              counts_out ? counts_out + (size_t)f * 12 : nullptr, scores_out ? scores_out + (size_t)f * 5 : nullptr,
                              sp_out ? sp_out + f : nullptr);
        }
        return KA_OK;
}

extern "C" int ka_cmp_fam_stats(ka_cmp_fam* h, double* stats_out)
{
        if (!h) return fail("ka_cmp_fam_stats: bad arguments");
        if (stats_out) std::copy_n(h->st, KA_CMP_STATS, stats_out);
        return KA_OK;
}
