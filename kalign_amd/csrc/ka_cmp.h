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
