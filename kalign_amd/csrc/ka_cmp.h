// ka_cmp.h -- scoring alignments against reference alignments (ka_cmp.hip kernels, ka_cmp.cpp host side): what the two
// units share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define KA_CMP_MAX_RES 32767       // residue index in an int16 map entry
#define KA_CMP_WALK 6              // the walk's counters per job: see the enum below
#define KA_CMP_SUMS 8              // a job's sums: the walk's six counters, tc_correct, tc_total
#define KA_CMP_STATS 4             // ka_cmp_stats: see include/kalign_amd.h
#define KA_CMP_DETAIL_STATS 5      // ka_cmp_detail_stats: see include/kalign_amd.h
#define KA_CMP_TI 16               // sequences i per tile of the pair walk
#define KA_CMP_TJ 32               // at most this many sequences j per tile (fewer when their rows do not fit the LDS budget)
#define KA_CMP_LDS 65536           // LDS budget of a walk workgroup for the staged rows (more only when one j row needs it)
#define KA_CMP_MAX_LDS 163840      // gfx950: LDS of one CU
#define KA_CMP_WALK_WGS 2048       // workgroups of a walk launch at most (8 per CU): more tiles are strided over
#define KA_CMP_CLASSES 4           // walk launches by LDS need: up to 16, 32 and 64 KiB (KA_CMP_LDS), and what is larger
#define KA_CMP_TCCHUNK 8           // consecutive job columns per wave of the TC pass and of the column pass at most

// res maps are stored with a row stride padded to 8 entries (16 bytes): a tile's rows copy as whole uint4s
static inline int ka_cmp_pad(int w) { return (w + 7) & ~7; }

// the walk's counters, summed over ordered pairs (i -> j, i != j) and the residues ri of i, with
// pR = resR[j][colR[i][ri]] and pT = resT[j][colT[i][ri]]:
enum {
        KA_CMP_REF_ALIGNED = 0,    // [pR >= 0]
        KA_CMP_TEST_ALIGNED = 1,   // [pT >= 0]
        KA_CMP_IDENT_ALIGNED = 2,  // [pR >= 0 && pR == pT]
        KA_CMP_IDENT_GAPS = 3,     // [pR < 0 && pT < 0]
        KA_CMP_REF_SCORED = 4,     // [pR >= 0 && scored[colR]]
        KA_CMP_COMMON_SCORED = 5,  // [pR >= 0 && pR == pT && scored[colR]]
};

// ---- the job table ----
// A handle holds one reference alignment or more (ka_cmp: one; ka_cmp_fam: one per family).  Their sequences, residues
// and columns are numbered flat over the handle, references in order.  A JOB is one test alignment scored against one
// reference: a score call of ka_cmp_fam has one job per family, a group of ka_cmp_score_batch has K jobs that share the
// one reference.  What counts the call's items -- test rows, job columns, tiles -- is numbered flat over the jobs of the
// call.  A kernel finds the reference or job of such a flat index by a search of an ascending first-index table
// (ka_fam_find, ka_msa.h).
struct KaCmpSide {                 // one alignment
        int W, Wp;                 // columns; res row stride (ka_cmp_pad)
        long long stride;          // bytes from a row to the next in the uploaded rows
        long long rowOff;          // first byte of its rows in the uploaded rows
        long long resOff;          // first entry of its res map [N][Wp]
};

struct KaCmpJob {
        int firstSeq, firstRes, firstCol;      // its reference: first sequence, flat residue and flat column in the handle
        int N;
        KaCmpSide r, t;                        // reference, test (a reference of the handle's table: r alone)
        long long colOff;                      // the test column of flat residue e of the reference is colT[colOff + e]
        int TJ, nTJ;                           // tile geometry of the walk: KA_CMP_TI x TJ sequences, nTJ j-tiles
};

struct KaCmpTab {
        int nRef, nJob;                        // references of the handle, jobs of the call
        int S, cols;                           // sequences and columns of the references
        int jobRows, jobCols;                  // test rows and job columns (a job has its reference's columns) of the call
        const KaCmpJob* refs;                  // [nRef]
        const KaCmpJob* jobs;                  // [nJob]
        const int* refSeq; const int* refCol;  // [nRef + 1] first sequence / column of a reference
        const int* jobRow; const int* jobCol;  // [nJob + 1] first test row / job column of a job
        const int* offs;                       // [S + 1] first flat residue of a sequence
        const int* lens;                       // [S]
        const int* seqOf;                      // [T] sequence of a flat residue, counted from its reference's first
        const uint8_t* rows;                   // uploaded rows of the side being mapped
        int* colR; int* colT;                  // column (in its own alignment) of a residue: colR[e], colT[job.colOff + e]
        int16_t* resR; int16_t* resT;          // res maps, at r.resOff / t.resOff
        int* colCnt;                           // [cols] residues in a reference column
        uint8_t* scored;                       // [cols]
        const float* frac;                     // [nRef] max_gap_frac
        const int* masks; const long long* maskOff;   // reference f's mask at masks + maskOff[f], or maskOff[f] < 0
        unsigned long long* sums;              // [nJob][KA_CMP_SUMS]
        // ---- a detail call (one job per reference, job k against reference k; unset in a score call) ----
        int T, tCols;                          // residues of the references; test columns of the call
        const int* tcolFirst;                  // [nJob + 1] first test column of a job
        int* detRes;                           // [3][T] per flat residue: the walk's REF_ALIGNED, TEST_ALIGNED, IDENT_ALIGNED
        // the column records: the call's tCols test columns, then the references' cols columns
        int* detColRes;                        // residues of the column (k)
        long long* detColCommon;               // plane 2 of detRes summed over the column's residues
        uint8_t* detColCorrect;                // k <= 1, or all k residues in one column of the other alignment
};

// ka_cmp.hip
void ka_cmp_run_maps(const KaCmpTab& a, int test, hipStream_t s);     // the references' maps (test 0) or the jobs' test maps
void ka_cmp_run_col_count(const KaCmpTab& a, hipStream_t s);
void ka_cmp_run_mask(const KaCmpTab& a, hipStream_t s);
// the tiles first[k] .. first[k + 1] - 1 (device, [nJob + 1]) of the jobs of one LDS class
// detail: every lane also adds its residue's three counts to the planes of a.detRes (zeroed by the caller)
int ka_cmp_run_walk(const KaCmpTab& a, const int* first, int nTiles, size_t lds, bool detail, hipStream_t s);
void ka_cmp_run_tc(const KaCmpTab& a, hipStream_t s);
// the column records of both sides, after the detailed walk
void ka_cmp_run_cols(const KaCmpTab& a, hipStream_t s);

// the doubles of one scored alignment from its exact counts, with the reference's expressions in its order: w = the walk's
// six sums, N sequences with T residues in all.  counts[12], scores[5] and sp (each optional) as ka_cmp_score hands them out.
// The one place these expressions live: every job ends here.
static inline void ka_cmp_finish(const long long* w, long long tcCorrect, long long tcTotal, int N, long long T, long long* counts,
                                 double* scores, float* sp)
{
        // every residue has N - 1 partners in each alignment: aligned or gap
        const uint64_t all = (uint64_t)(N - 1) * (uint64_t)T;
        // struct cmp_stats, in its field order
        const uint64_t refAl = (uint64_t)w[KA_CMP_REF_ALIGNED], refGap = all - refAl;
        const uint64_t identAl = (uint64_t)w[KA_CMP_IDENT_ALIGNED], identGap = (uint64_t)w[KA_CMP_IDENT_GAPS];
        const uint64_t testAl = (uint64_t)w[KA_CMP_TEST_ALIGNED], testGap = all - testAl;
        // struct detailed_pair_stats
        const int64_t refScored = w[KA_CMP_REF_SCORED], testPairs = w[KA_CMP_TEST_ALIGNED];
        const int64_t commonScored = w[KA_CMP_COMMON_SCORED], commonAll = w[KA_CMP_IDENT_ALIGNED];
        if (counts) {
                counts[0] = (long long)refAl; counts[1] = (long long)refGap; counts[2] = (long long)identAl; counts[3] = (long long)identGap;
                counts[4] = (long long)testAl; counts[5] = (long long)testGap;
                counts[6] = refScored; counts[7] = testPairs; counts[8] = commonScored; counts[9] = commonAll;
                counts[10] = tcCorrect; counts[11] = tcTotal;
        }
        // kalign_msa_compare (msa_cmp.c:120-123)
        const double sa = (double)(identAl + identGap);
        const double sb = (double)(refAl + refGap);
        const double spd = 100.0 * sa / sb;
        if (sp) *sp = (float)spd;
        // compare_with_mask_helper (msa_cmp.c:370-398)
        const double recall = refScored > 0 ? (double)commonScored / (double)refScored : 0.0;
        const double precision = testPairs > 0 ? (double)commonAll / (double)testPairs : 0.0;
        const double f1 = recall + precision > 0.0 ? 2.0 * recall * precision / (recall + precision) : 0.0;
        const double tcv = tcTotal > 0 ? (double)(int)tcCorrect / (double)(int)tcTotal : 0.0;
        if (scores) {
                scores[0] = recall; scores[1] = precision; scores[2] = f1; scores[3] = tcv; scores[4] = spd;
        }
}
