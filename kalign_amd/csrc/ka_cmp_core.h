// ka_cmp_core.h -- the host core of the comparison stage (ka_cmp.cpp): the references of a handle on the device and the
// score sequence over a call's jobs.  ka_cmp (ka_cmp.cpp) and ka_cmp_fam (ka_cmp_fam.cpp) are fronts over it.
#pragma once
#include <functional>
#include <memory>
#include "ka_ctx.h"
#include "ka_cmp.h"
#include "ka_msa.h"

// a front's rows to `dst` in the layout it has stated (stream-ordered); KA_OK or KA_FAIL
typedef std::function<int(uint8_t* dst, hipStream_t s)> KaCmpUpload;

struct KaCmpCore {
        int device = 0;
        hipStream_t stream = nullptr;
        int S = 0, T = 0, cols = 0;            // sequences, residues and columns of the references
        std::vector<KaCmpJob> refs;            // the references (r side)
        std::vector<int> lens, offs;           // [S], [S + 1]
        DevBuf<KaCmpJob> dRefs, dJobs;
        DevBuf<int> dRefFirst, dJobFirst, dOffs, dLens, dSeqOf, dColR, dColT, dColCnt, dMasks;
        DevBuf<int16_t> dResR, dResT;
        DevBuf<uint8_t> dRows, dScored;
        DevBuf<float> dFrac;
        DevBuf<long long> dMaskOff;
        DevBuf<unsigned long long> dSums;
        hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
        double st[KA_CMP_STATS] = {};          // ka_cmp_stats; score() adds its stages to st[1..3]

        ~KaCmpCore();
        int attach(ka_ctx* ctx);               // the context's device and stream
        void close();                          // waits for the stream
        // Errors read "<who>: ..." or, about one reference or job with `item` given, "<who>: <item> <k>: ...".
        // The rows of an alignment of width W lie W + pad bytes apart where `upload` puts them, alignments back to back.
        // nRef references, reference f the sequences first[f] .. first[f + 1] - 1 (checked by the front): maps, column
        // counts, every column scored
        int create(const char* who, const char* item, int nRef, const int* first, const int* lens, const int* widths, int pad, const KaCmpUpload& upload);
        // reference f's columns: its mask at masks + maskOff[f] (nMask ints in all), or with maskOff[f] < 0 the float rule of frac[f]
        int set_rule(const char* who, const float* frac, const int* masks, const long long* maskOff, long long nMask);
        // nJob jobs, job k a test of widths[k] columns against reference refOf[k] (NULL: k); outputs as ka_cmp_score_batch's
        int score(const char* who, const char* item, int nJob, const int* refOf, const int* widths, int pad, const KaCmpUpload& upload,
                  long long* counts, double* scores, float* sp);
        // one job per reference (job f a test of widths[f] columns against reference f): the counts of every residue and
        // the records of every test and reference column, as ka_cmp_fam_detail hands them out (each optional).  Fills dst
        // and leaves st alone.  The front zeroes dst before its checks: a refused call reads as no launch
        int detail(const char* who, const char* item, const int* widths, int pad, const KaCmpUpload& upload, int* resCounts, int* tcolRes,
                   long long* tcolCommon, uint8_t* tcolCorrect, int* rcolRes, long long* rcolCommon, uint8_t* rcolCorrect);
        double dst[KA_CMP_DETAIL_STATS] = {};  // ka_cmp_detail_stats: of the last detail call

private:
        // what a call numbers flat over its jobs: a first-index table each, [nJob + 1], back to back in `first`
        enum { ROWS = 0, COLS = 1, TCOLS = 2, TILES = 3, TABLES = TILES + KA_CMP_CLASSES };
        struct Call {                          // a call's jobs on the device, their test maps launched
                int nJob = 0;
                std::vector<KaCmpJob> jobs;
                std::vector<int> first;        // [TABLES][nJob + 1]
                size_t classLds[KA_CMP_CLASSES] = {};
                KaCmpTab a{};
                int last(int table) const { return first[(size_t)table * (nJob + 1) + nJob]; }
        };
        // the steps score() and detail() share: the job table, the upload and the test maps (events 0, 1 around the
        // maps); then the walk of every LDS class in use (event 2 behind it).  *launches counts the kernels
        int begin(const char* who, const char* item, int nJob, const int* refOf, const int* widths, int pad, const KaCmpUpload& upload, Call& c,
                  int* launches);
        int walk(const char* who, const Call& c, bool detailed, int* launches);
        float ms(int a, int b) { float m = 0.0f; (void)hipEventElapsedTime(&m, ev[a], ev[b]); return m; }
        KaCmpTab tab() const;                  // the handle's side of the table
        DevBuf<uint8_t> dDet;                  // a detail call's outputs, one block: see detail()
};
