// ka_cmp.cpp -- host side of scoring alignments against a reference alignment (kalign_msa_compare*, lib/src/msa_cmp.c):
// the ka_cmp handle of the C ABI.
//
// The reference alignment's position maps and per-column residue counts are built once (ka_cmp_create); each test
// alignment gets its own maps, then the pair walk and the TC pass (ka_cmp.hip).  The device returns exact integer counts;
// the final doubles are computed on the host with the reference's expressions, in its order (ka_cmp_finish, ka_cmp.h).
//
// Unlike the reference, the two alignments must hold the same sequences: numseq rows each, row s with lens[s] letters
// (the reference reads out of bounds otherwise).  Two sequences at least.
#include "ka_ctx.h"
#include "ka_cmp.h"
#include "ka_msa.h"

int ka_ctx_device_stream(ka_ctx* c, int* device, hipStream_t* stream);    // (library-internal: ka_api.cpp)

namespace {

constexpr int kGroup = 32;         // test alignments per device pass of ka_cmp_score_batch

} // namespace

struct ka_cmp {
        int device = 0;
        hipStream_t stream = nullptr;
        KaSeqSet q;
        int WR = 0, WRp = 0;
        DevBuf<int> dSeqOf, dColR, dColCnt, dMask, dColT, dTWp;
        DevBuf<int16_t> dResR, dResT;
        DevBuf<uint8_t> dRows, dScored;
        DevBuf<long long> dTResOff, dSlab, dSums;
        DevBuf<unsigned long long> dTc;
        hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
        double st[KA_CMP_STATS] = {};

        ~ka_cmp()
        {
                for (auto& e : ev)
                        if (e) (void)hipEventDestroy(e);
                q.release();
                dSeqOf.release(); dColR.release(); dColCnt.release(); dMask.release();
                dColT.release(); dTWp.release(); dResR.release(); dResT.release(); dRows.release(); dScored.release();
                dTResOff.release(); dSlab.release(); dSums.release(); dTc.release();
        }

        float ms(int a, int b) { float m = 0.0f; (void)hipEventElapsedTime(&m, ev[a], ev[b]); return m; }

        int score(int K, const uint8_t* const* rows, const long long* strides, const int* alnlens, long long* counts, double* scores, float* sp);
};

// K <= kGroup test alignments, checked by the caller
int ka_cmp::score(int K, const uint8_t* const* rows, const long long* strides, const int* alnlens, long long* counts, double* scores, float* sp)
{
        const int N = q.N, T = q.T;
        std::vector<long long> rowOff(K + 1, 0), resOff(K + 1, 0);
        std::vector<int> wp(K);
        int maxWTp = 0;
        for (int k = 0; k < K; k++) {
                wp[k] = ka_cmp_pad(alnlens[k]);
                maxWTp = std::max(maxWTp, wp[k]);
                rowOff[k + 1] = rowOff[k] + (long long)N * alnlens[k];
                resOff[k + 1] = resOff[k] + (long long)N * wp[k];
        }
        // the walk stages TJ rows of both maps in LDS: as many as the budget holds, one at least
        const size_t rowBytes = (size_t)(WRp + maxWTp) * sizeof(int16_t);
        int TJ = (int)std::min<size_t>(KA_CMP_TJ, KA_CMP_LDS / rowBytes);
        TJ = std::max(1, std::min(TJ, N));
        const size_t lds = (size_t)TJ * rowBytes;
        if (lds > KA_CMP_MAX_LDS - 1024)
                return fail("ka_cmp_score: reference width " + std::to_string(WR) + " and test width " + std::to_string(maxWTp) +
                            " together exceed the LDS of one CU (one row of each is staged)");
        const int nTI = (N + KA_CMP_TI - 1) / KA_CMP_TI, nTJ = (N + TJ - 1) / TJ;
        const int nTiles = nTI * nTJ;
        const int gridX = std::max(1, std::min(nTiles, (KA_CMP_GRID + K - 1) / K));
        if (dRows.alloc((size_t)rowOff[K]) || dColT.alloc((size_t)K * std::max(T, 1)) || dResT.alloc((size_t)resOff[K]) ||
            dTResOff.alloc(K) || dTWp.alloc(K) || dSlab.alloc((size_t)K * gridX * KA_CMP_WALK) || dSums.alloc((size_t)K * KA_CMP_WALK) ||
            dTc.alloc((size_t)2 * K))
                return fail("ka_cmp_score: out of device memory");
        for (int k = 0; k < K; k++)
                if (ka_msa_upload_rows(q, dRows.p + rowOff[k], rows[k], strides[k], alnlens[k], stream)) return KA_FAIL;
        HIPCHK(hipMemcpyAsync(dTResOff.p, resOff.data(), sizeof(long long) * K, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dTWp.p, wp.data(), sizeof(int) * K, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemsetAsync(dTc.p, 0, sizeof(unsigned long long) * 2 * K, stream));
        HIPCHK(hipEventRecord(ev[0], stream));
        for (int k = 0; k < K; k++)
                ka_msa_launch_maps(dRows.p + rowOff[k], alnlens[k], alnlens[k], wp[k], q, dColT.p + (long long)k * T, dResT.p + resOff[k], stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], stream));
        KaCmpArgs a{};
        a.N = N; a.T = T; a.offs = q.dOffs; a.seqOf = dSeqOf.p;
        a.colR = dColR.p; a.resR = dResR.p; a.WR = WR; a.WRp = WRp; a.scored = dScored.p;
        a.colT = dColT.p; a.resT = dResT.p; a.tResOff = dTResOff.p; a.tWp = dTWp.p; a.maxWTp = maxWTp;
        a.TJ = TJ; a.nTI = nTI; a.nTJ = nTJ;
        a.slab = dSlab.p; a.sums = dSums.p; a.colCnt = dColCnt.p; a.tc = dTc.p;
        if (ka_cmp_launch_walk(a, K, gridX, lds, stream)) return fail("ka_cmp_score: the walk's LDS (" + std::to_string(lds) + " bytes) was refused");
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[2], stream));
        ka_cmp_launch_tc(a, K, stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[3], stream));
        std::vector<long long> sums((size_t)K * KA_CMP_WALK);
        std::vector<unsigned long long> tc((size_t)2 * K);
        HIPCHK(hipMemcpyAsync(sums.data(), dSums.p, sizeof(long long) * sums.size(), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(tc.data(), dTc.p, sizeof(unsigned long long) * tc.size(), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        st[1] += ms(0, 1); st[2] += ms(1, 2); st[3] += ms(2, 3);
        for (int k = 0; k < K; k++)
                ka_cmp_finish(&sums[(size_t)k * KA_CMP_WALK], (long long)tc[2 * k], (long long)tc[2 * k + 1], N, T,
                              counts ? counts + (size_t)k * 12 : nullptr, scores ? scores + (size_t)k * 5 : nullptr, sp ? sp + k : nullptr);
        return KA_OK;
}

extern "C" int ka_cmp_create(ka_ctx* ctx, int numseq, const int* lens, const uint8_t* ref_rows, long long row_stride, int alnlen, ka_cmp** out)
{
        if (!ctx || !out || !lens) return fail("ka_cmp_create: bad arguments");
        *out = nullptr;
        if (numseq < 2) return fail("ka_cmp_create: " + std::to_string(numseq) + " sequences; a comparison needs two at least");
        std::unique_ptr<ka_cmp> h(new ka_cmp);
        if (ka_ctx_device_stream(ctx, &h->device, &h->stream)) return fail("ka_cmp_create: bad context");
        HIPCHK(hipSetDevice(h->device));
        const std::string why = "the position maps hold at most " + std::to_string(KA_CMP_MAX_RES);
        if (h->q.init("ka_cmp_create", numseq, lens, KA_CMP_MAX_RES, why.c_str())) return KA_FAIL;
        if (ka_msa_check_rows("ka_cmp_create", h->q, ref_rows, row_stride, alnlen)) return KA_FAIL;
        h->WR = alnlen;
        h->WRp = ka_cmp_pad(alnlen);
        if ((size_t)h->WRp * 2 * sizeof(int16_t) > KA_CMP_MAX_LDS - 1024)
                return fail("ka_cmp_create: reference width " + std::to_string(alnlen) + " exceeds the LDS of one CU (a row of each alignment is staged)");
        const int T = h->q.T;
        for (auto& e : h->ev) HIPCHK(hipEventCreate(&e));
        std::vector<int> seqOf((size_t)std::max(T, 1), 0);
        for (int s = 0; s < numseq; s++) std::fill_n(seqOf.begin() + h->q.offs[s], lens[s], s);
        if (h->dSeqOf.alloc(seqOf.size()) || h->dColR.alloc((size_t)std::max(T, 1)) ||
            h->dResR.alloc((size_t)numseq * h->WRp) || h->dColCnt.alloc(alnlen) || h->dScored.alloc(alnlen) || h->dRows.alloc((size_t)numseq * alnlen))
                return fail("ka_cmp_create: out of device memory");
        HIPCHK(hipMemcpyAsync(h->dSeqOf.p, seqOf.data(), sizeof(int) * seqOf.size(), hipMemcpyHostToDevice, h->stream));
        if (ka_msa_upload_rows(h->q, h->dRows.p, ref_rows, row_stride, alnlen, h->stream)) return KA_FAIL;
        HIPCHK(hipEventRecord(h->ev[0], h->stream));
        ka_msa_launch_maps(h->dRows.p, alnlen, alnlen, h->WRp, h->q, h->dColR.p, h->dResR.p, h->stream);
        ka_cmp_launch_col_count(h->dResR.p, alnlen, h->WRp, numseq, h->dColCnt.p, h->stream);
        ka_cmp_launch_mask(h->dColCnt.p, alnlen, numseq, -1.0f, nullptr, h->dScored.p, h->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev[1], h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->st[0] = h->ms(0, 1);
        *out = h.release();
        return KA_OK;
}

extern "C" void ka_cmp_destroy(ka_cmp* h)
{
        if (!h) return;
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        delete h;
}

extern "C" int ka_cmp_set_mask(ka_cmp* h, float max_gap_frac, const int* mask, int n_cols)
{
        if (!h) return fail("ka_cmp_set_mask: bad arguments");
        if (mask && n_cols != h->WR)
                return fail("ka_cmp_set_mask: mask length " + std::to_string(n_cols) + " != reference alignment length " + std::to_string(h->WR));
        HIPCHK(hipSetDevice(h->device));
        if (mask) {
                if (h->dMask.alloc(h->WR)) return fail("ka_cmp_set_mask: out of device memory");
                HIPCHK(hipMemcpyAsync(h->dMask.p, mask, sizeof(int) * h->WR, hipMemcpyHostToDevice, h->stream));
        }
        ka_cmp_launch_mask(h->dColCnt.p, h->WR, h->q.N, max_gap_frac, mask ? h->dMask.p : nullptr, h->dScored.p, h->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        return KA_OK;
}

extern "C" int ka_cmp_score_batch(ka_cmp* h, int n_tests, const uint8_t* const* test_rows, const long long* row_strides, const int* alnlens,
                                  long long* counts_out, double* scores_out, float* sp_out)
{
        if (!h || n_tests < 0 || (n_tests > 0 && (!test_rows || !row_strides || !alnlens))) return fail("ka_cmp_score_batch: bad arguments");
        for (int k = 0; k < n_tests; k++) {
                const std::string who = "ka_cmp_score: test " + std::to_string(k);
                if (ka_msa_check_rows(who.c_str(), h->q, test_rows[k], row_strides[k], alnlens[k])) return KA_FAIL;
        }
        HIPCHK(hipSetDevice(h->device));
        h->st[1] = h->st[2] = h->st[3] = 0.0;
        for (int k0 = 0; k0 < n_tests; k0 += kGroup) {
                const int K = std::min(kGroup, n_tests - k0);
                if (h->score(K, test_rows + k0, row_strides + k0, alnlens + k0, counts_out ? counts_out + (size_t)k0 * 12 : nullptr,
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
        if (stats_out) std::copy_n(h->st, KA_CMP_STATS, stats_out);
        return KA_OK;
}
