// ka_sum.h -- summaries and trimming of the finished rows of a batch of families (ka_sum.hip kernels, ka_sum.cpp host
// side): what the two units share.
//
// The rule for a byte: a gap is the byte `gap`; every other byte is a character and is compared as a byte (upper and lower
// case differ).  This is kalign.utils' rule, not the isalpha rule of ka_msa.h: '.' and '*' are characters here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define KA_SUM_TILE 64             // columns per tile of the column table: one lane of a wave per column
#define KA_SUM_BINS 256            // a tile's histogram: KA_SUM_BINS x KA_SUM_TILE counters of 32 bits (64 KiB of LDS), bin-major
#define KA_SUM_THREADS 512         // threads of a column-table workgroup: its waves deal the family's rows among them
#define KA_SUM_PARTS (KA_SUM_THREADS / KA_SUM_TILE)   // the bins are reduced in this many parts, a wave each (32 bins: one word of the presence mask)
#define KA_SUM_SCAN 256            // columns per step of the per-family scan (one per thread)
#define KA_SUM_CHUNK 256           // output columns per wave of the row gather: four bytes per lane
#define KA_SUM_FAMSUMS 4           // a family's sums from the device: see the enum below
#define KA_SUM_STATS 6             // ka_sum_fam_stats: see include/kalign_amd.h
// the identity matrices (sum_identity): a workgroup of four waves owns a T x T tile of pairs of rows of one family, a wave a
// quarter of it (8 x 8 lanes), a lane KA_SUM_IDM_RT x KA_SUM_IDM_RT pairs
// (both measured against 4 x 4 pairs and 256 columns: DESIGN.md 4p; -DKA_SUM_IDM_RT=4 -DKA_SUM_IDM_CHUNK=256 builds those)
#ifndef KA_SUM_IDM_RT
#define KA_SUM_IDM_RT 2
#endif
#define KA_SUM_IDM_T (16 * KA_SUM_IDM_RT)      // rows per side of a tile of pairs: 32
#ifndef KA_SUM_IDM_CHUNK
#define KA_SUM_IDM_CHUNK 128       // columns staged in LDS per step over the width
#endif
#define KA_SUM_IDM_THREADS 256
#define KA_SUM_IDM_STATS 3         // ka_sum_fam_identity_stats: see include/kalign_amd.h

// the walk along rows (sum_gap_rows, sum_ungap): a wave per row, KA_SUM_CHUNK columns a step as four ballots of 64
#define KA_SUM_GAP_THREADS 1024    // sum_gap_rows: sixteen waves, sixteen consecutive rows, per workgroup
#define KA_SUM_ROW_THREADS 256     // sum_ungap: four waves, four rows, per workgroup
#define KA_SUM_ROWREC 4            // a row's record: see the enum below
#define KA_SUM_GAPSUMS 5           // a family's sums of the gap structure: see the enum below
#define KA_SUM_GAP_COUNTS 8        // ka_sum_fam_gaps' counts per family, KA_SUM_GAP_VALUES its doubles: see include/kalign_amd.h
#define KA_SUM_GAP_VALUES 7
#define KA_SUM_GAP_STATS 6         // ka_sum_fam_gap_stats: see include/kalign_amd.h

enum {
        KA_ROW_CHARS = 0,          // characters of the row
        KA_ROW_LEADING = 1,        // gap columns before its first character (W in an all-gap row)
        KA_ROW_TRAILING = 2,       // gap columns after its last character (W in an all-gap row)
        KA_ROW_BLOCKS = 3,         // maximal runs of gaps
};

enum {
        KA_GAP_CHARS = 0,          // sum over the family's rows of the characters
        KA_GAP_BLOCKS = 1,         // ... of the gap blocks
        KA_GAP_TERMINAL = 2,       // ... of leading + trailing (an all-gap row adds 2 W)
        KA_GAP_INTERNAL = 3,       // ... of max(0, gaps - leading - trailing)
        KA_GAP_GAPPY = 4,          // columns with 2 nGap > N
};

enum {
        KA_SUM_GAPS = 0,           // gap bytes
        KA_SUM_CONSERVED = 1,      // columns with a character and one distinct character
        KA_SUM_MATCHING = 2,       // sum over columns and characters a of n_a (n_a - 1) / 2
        KA_SUM_COMPARED = 3,       // sum over columns of k (k - 1) / 2, k the column's characters
};

// one family: N rows of W columns from rows + rowOff, W + 1 bytes apart; its columns are firstCol .. firstCol + W - 1 of
// the batch, its consensus row starts at firstCol + (its number) in a packed consensus
struct KaSumFam {
        int N, W;
        int firstCol;
        int chunks;                // gather chunks of one of its rows: ceil((W + 1) / KA_SUM_CHUNK)
        long long rowOff;
};

struct KaSumTab {
        int nFam, cols, nTiles;
        int nItems;                            // gather items: (row, chunk) pairs over the batch
        uint8_t gap;
        const KaSumFam* fams;                  // [nFam]
        const int* tileFirst;                  // [nFam + 1] first column tile of a family
        const int* colFirst;                   // [nFam + 1] first column
        const int* itemFirst;                  // [nFam + 1] first gather item
        const uint8_t* rows;
        // the column table
        int* nGap; int* nDistinct; int* topCount; uint8_t* topChar; long long* samePairs;   // [cols]
        unsigned long long* famSums;           // [nFam][KA_SUM_FAMSUMS]
        unsigned* present;                     // [nFam][8]: bit b of the 256 is set when byte b is a character of the family
        // a call's rule and results
        const double* thr;                     // [nFam]
        const uint8_t* ambiguous;              // [nFam]
        const int* masks; const long long* maskOff;   // family f's mask at masks + maskOff[f], or maskOff[f] < 0 (masks NULL: none)
        int* keep;                             // [cols] 0 / 1
        int* src;                              // [cols] the kept columns of family f, in order, from src + firstCol
        int* newW;                             // [nFam] kept columns
        long long* outOff;                     // [nFam] first byte of a family's compacted rows
        uint8_t* out;                          // consensus rows, or compacted rows
};

// the identity matrices of the batch: family f's N x N block, row-major, starts at entry entFirst[f] of each of the three
// matrices; its upper-triangle tiles (tile row <= tile column) are tileFirst[f] .. tileFirst[f + 1] - 1 of `tiles`
struct KaIdmTab {
        int nFam, nTiles;
        uint8_t gap;
        const KaSumFam* fams;                  // [nFam]
        const int* tileFirst;                  // [nFam + 1]
        const int* entFirst;                   // [nFam + 1] (the batch holds fewer than 2^31 entries)
        const unsigned* tiles;                 // [nTiles] tile row << 16 | tile column, inside the family
        const uint8_t* rows;
        long long bytes;                       // of the rows: nothing from there on is read
        int* matches; int* compared;           // [entries]
        double* identity;                      // [entries]
};

// the walk along the rows of the batch: rows are numbered flat over the families, family f's are rowFirst[f] ..
// rowFirst[f + 1] - 1
struct KaGapTab {
        int nFam, nRows, cols;
        uint8_t gap;
        const KaSumFam* fams;                  // [nFam]
        const int* rowFirst;                   // [nFam + 1]
        const int* colFirst;                   // [nFam + 1]
        const uint8_t* rows;
        const int* nGap;                       // [cols] of the column table
        int* recs;                             // [nRows][KA_SUM_ROWREC]
        unsigned long long* sums;              // [nFam][KA_SUM_GAPSUMS] (zeroed first by the caller)
        // the ungapped rows: row r's characters, in order, from out + off[r]; off[nRows] bytes in all
        const long long* off;                  // [nRows + 1]
        uint8_t* out;
};

// ka_sum.hip: every launcher adds the kernels it launches to *launches
int ka_sum_run_columns(const KaSumTab& a, hipStream_t s, int* launches);     // the column table, the family sums and the presence masks (zeroed first by the caller); 1: the LDS was refused
void ka_sum_run_consensus(const KaSumTab& a, hipStream_t s, int* launches);
void ka_sum_run_keep(const KaSumTab& a, hipStream_t s, int* launches);       // keep flags, then the per-family scan: src, newW
void ka_sum_run_gather(const KaSumTab& a, hipStream_t s, int* launches);     // outOff over the families, then the rows
int ka_sum_run_identity(const KaIdmTab& a, hipStream_t s, int* launches);     // the three matrices, both triangles; 1: the LDS was refused
void ka_sum_run_gaps(const KaGapTab& a, hipStream_t s, int* launches);       // the row records and the families' five sums: the row pass, then the gappy columns
void ka_sum_run_ungap(const KaGapTab& a, hipStream_t s, int* launches);      // the characters of every row, packed at a.off
