// ka_cmp.h -- scoring an alignment against a reference alignment (ka_cmp.hip kernels, ka_cmp.cpp host side): what the
// two units share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define KA_CMP_MAX_RES 32767       // residue index in an int16 map entry
#define KA_CMP_WALK 6              // the walk's counters per test: see KaCmpArgs
#define KA_CMP_STATS 4             // ka_cmp_stats: see include/kalign_amd.h
#define KA_CMP_TI 16               // sequences i per tile of the pair walk
#define KA_CMP_TJ 32               // at most this many sequences j per tile (fewer when their rows do not fit the LDS budget)
#define KA_CMP_LDS 65536           // LDS budget of a walk workgroup for the staged rows (more only when one j row needs it)
#define KA_CMP_MAX_LDS 163840      // gfx950: LDS of one CU
#define KA_CMP_GRID 1024           // workgroups of the walk per test at most (each then walks several tiles)

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

struct KaCmpArgs {
        int N, T;                  // sequences, residues
        const int* offs;           // [N + 1] first residue of sequence s in the flat numbering (offs[N] = T)
        const int* seqOf;          // [T] sequence of a flat residue
        const int* colR;           // [T] reference column of residue e
        const int16_t* resR;       // [N][WRp] residue of s at reference column c, or -1
        int WR, WRp;
        const uint8_t* scored;     // [WR] column mask of the reference
        const int* colT;           // test k at k * T
        const int16_t* resT;       // test k at tResOff[k]: [N][tWp[k]]
        const long long* tResOff;  // [K]
        const int* tWp;            // [K]
        int maxWTp;                // widest test (LDS layout)
        int TJ, nTI, nTJ;          // tile geometry: KA_CMP_TI x TJ sequences
        long long* slab;           // [K][gridDim.x][KA_CMP_WALK]
        long long* sums;           // [K][KA_CMP_WALK]
        const int* colCnt;         // [WR] residues in reference column c
        unsigned long long* tc;    // [K][2] tc_correct, tc_total
};

// ka_cmp.hip
void ka_cmp_launch_col_count(const int16_t* res, int W, int Wp, int N, int* colCnt, hipStream_t s);
void ka_cmp_launch_mask(const int* colCnt, int W, int N, float maxGapFrac, const int* mask, uint8_t* scored, hipStream_t s);
int ka_cmp_launch_walk(const KaCmpArgs& a, int K, int gridX, size_t lds, hipStream_t s);
void ka_cmp_launch_tc(const KaCmpArgs& a, int K, hipStream_t s);

// the doubles of one scored alignment from its exact counts, with the reference's expressions in its order: w = the walk's
// six sums, N sequences with T residues in all.  counts[12], scores[5] and sp (each optional) as ka_cmp_score hands them out.
// The one place these expressions live: ka_cmp_score and ka_cmp_fam_score both end here.
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

// ---- a batch of families, each with its own reference and test alignment (ka_cmp_fam.hip kernels, ka_cmp_fam.cpp host side) ----
// Sequences, residues and reference columns are numbered flat over the batch, families in order; a family's kernels find
// their family from such a flat index by a search of the ascending first-index tables.
#define KA_CMPF_GRID 2048          // workgroups of a walk launch at most (8 per CU): more tiles are strided over
#define KA_CMPF_CLASSES 4          // walk launches by LDS need: up to 16, 32 and 64 KiB (KA_CMP_LDS), and what is larger
#define KA_CMPF_TCCHUNK 8          // consecutive flat reference columns per wave of the TC pass

struct KaCmpSide {                 // one alignment of a family
        int W, Wp;                 // columns; res row stride (ka_cmp_pad)
        long long rowOff;          // first byte of the family's rows in the packed rows (rows W + 1 bytes apart)
        long long resOff;          // first entry of the family's res map [N][Wp]
};

struct KaCmpFam {
        int firstSeq, firstRes, firstCol;      // first sequence, flat residue and flat reference column of the family
        int N;
        KaCmpSide r, t;                        // reference, test
        int TJ, nTJ;                           // tile geometry of the walk: KA_CMP_TI x TJ sequences, nTJ j-tiles
};

struct KaCmpFamArgs {
        int nFam, S, cols;                     // families, sequences, flat reference columns
        const KaCmpFam* fams;                  // [nFam]
        const int* firstSeq;                   // [nFam + 1]
        const int* firstCol;                   // [nFam + 1]
        const int* offs;                       // [S + 1] first flat residue of a sequence
        const int* lens;                       // [S]
        const int* seqOf;                      // [T] sequence of a flat residue, counted from its family's first
        const uint8_t* rows;                   // packed rows of the side being mapped
        int* colR; int* colT;                  // [T] column (in its family's alignment) of a flat residue
        int16_t* resR; int16_t* resT;          // res maps, family f at fams[f].r.resOff / .t.resOff
        int* colCnt;                           // [cols] residues in a reference column
        uint8_t* scored;                       // [cols]
        const float* frac;                     // [nFam] max_gap_frac
        const int* masks; const long long* maskOff;   // family f's mask at masks + maskOff[f], or maskOff[f] < 0
        unsigned long long* sums;              // [nFam][KA_CMPF_SUMS]: the walk's six counters, tc_correct, tc_total
};
#define KA_CMPF_SUMS 8

// ka_cmp_fam.hip
void ka_cmpf_launch_maps(const KaCmpFamArgs& a, int test, hipStream_t s);
void ka_cmpf_launch_col_count(const KaCmpFamArgs& a, hipStream_t s);
void ka_cmpf_launch_mask(const KaCmpFamArgs& a, hipStream_t s);
// the tiles first[f] .. first[f + 1] - 1 (device, [nFam + 1]) of the families of one LDS class
int ka_cmpf_launch_walk(const KaCmpFamArgs& a, const int* first, int nTiles, size_t lds, hipStream_t s);
void ka_cmpf_launch_tc(const KaCmpFamArgs& a, hipStream_t s);
