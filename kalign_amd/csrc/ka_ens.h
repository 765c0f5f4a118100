// ka_ens.h -- the ensemble consensus stage (ka_ens.hip and ka_poar.hip kernels; ka_ens.cpp, ka_ens_fam.cpp host side): what the units share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#define KA_ENS_MAX_RUNS 32
#define KA_ENS_MAX_RES 4096        // residue index < 4096: the reference's POAR key ri << 20 | rj aliases from there on
#define KA_ENS_STATS 10            // ka_ens_stats: see include/kalign_amd.h
#define KA_ENS_TABLE_STATS 6       // ka_ens_table_stats
#define KA_ENS_JCHUNK 16           // j per workgroup of the support walk (4 waves, one j at a time each)
#define KA_ENS_FAM_STATS 21        // ka_ens_fam_stats

enum { KA_ENS_SCORE = 0, KA_ENS_CONF = 1, KA_ENS_COUNT = 2, KA_ENS_WRITE = 3 };

struct KaEnsArgs {
        const int* offs;           // [N + 1] first residue of sequence s in the flat residue numbering
        const int* lens;           // [N]
        int N, R, T, maxlen;       // sequences, members, residues, longest sequence
        const int* col;            // [R][T]  col[k * T + offs[s] + r] = column of residue r of s in member k
        const int16_t* res;        // member k at resOff[k]: [N][W[k]], residue of s at column c or -1
        long long resOff[KA_ENS_MAX_RUNS];
        int W[KA_ENS_MAX_RUNS];
        // the alignment X of SCORE / CONF: its own tables
        const int* colX;           // [T]
        const int16_t* resX;       // [N][Wx]
        int Wx;
        int i0, i1;                // sequences i of this launch
        int colInLds;              // member columns of sequence i staged in LDS (else read where they lie)
        int level;                 // COUNT / WRITE: support value of the candidates
        unsigned long long* score; // SCORE: sum of (support - 1), two's complement
        int* supSum;               // CONF: [T] sum of support over the residue's partners
        int* nPair;                // CONF: [T] number of partners
        int* cnt;                  // COUNT: [N * N] candidates of pair (i, j)
        const long long* pairOff;  // WRITE: [N * N] first slot of pair (i, j), relative to the row
        const long long* rowBase;  // WRITE: [N] first slot of row i, relative to this chunk
        int2* out;                 // WRITE: (element of i, element of j)
        // the POAR table (ka_poar.hip): built from the members, or the source of support of a handle opened from one
        uint2* entOut;             // table WRITE: (key = ri << 20 | rj, mask: bit k = member k holds the pair)
        const long long* pairStart;// [N * (N - 1) / 2 + 1] first entry of pair (i, j), i < j, pairs in (i, j) order
        const uint2* ent;          // the entries, keys ascending inside a pair
        // the table algebra (poar_merge, poar_select): a new table from ent (and entB), its pairs' first entries known after COUNT
        const long long* pairStartB; // merge: the second table, whose member bits go above the first's shift bits
        const uint2* entB;
        int shift;                 // merge: members of the first table
        int nSel;                  // select: members kept; new bit t = old bit sel[t]
        unsigned char sel[KA_ENS_MAX_RUNS];
        const long long* outStart; // merge / select WRITE: [N * (N - 1) / 2 + 1] first entry of pair (i, j) in entOut
};

__device__ __forceinline__ int ens_wave_incl_scan(int v, int lane)
{
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(v, o, 64);
                if (lane >= o) v += t;
        }
        return v;
}

// index of pair (i, j), i < j, in the table's order (poar.c's pair_index)
__host__ __device__ inline long long ka_poar_pair(int i, int j, int N) { return (long long)i * N - (long long)i * (i + 1) / 2 + (j - i - 1); }

// ka_poar.hip: the walk's modes, over rows i0 .. i1 of one family (a workgroup per sequence i and KA_ENS_JCHUNK sequences j)
void ka_poar_launch_table(int mode, const KaEnsArgs& a, hipStream_t s);       // COUNT / WRITE: the members' table, pair by pair
void ka_poar_launch_level(int mode, const KaEnsArgs& a, hipStream_t s);       // COUNT / WRITE over a loaded table: the entries with
                                                                              // popcount == level as candidates; level 0: every entry, as it is
void ka_poar_launch_lookup(int mode, const KaEnsArgs& a, hipStream_t s);      // SCORE / CONF with support read from a loaded table
void ka_poar_launch_merge(int mode, const KaEnsArgs& a, hipStream_t s);       // COUNT / WRITE: the union of two tables, the second's bits shifted
void ka_poar_launch_select(int mode, const KaEnsArgs& a, hipStream_t s);      // COUNT / WRITE: a table with the member bits sel[], emptied entries dropped
// pairStart[pair (i, j)] = rowBase[i - i0] + pairOff[(i - i0) * N + j] for rows i0 .. i1: a counted block's offsets in the table's own layout
void ka_poar_launch_pair_start(const long long* pairOff, const long long* rowBase, int i0, int i1, int N, long long* pairStart, hipStream_t s);
// ka_poar.cpp: the checks of ka_poar_check_image; also fills the pairs' first entries (n_pairs + 1) when asked
int ka_poar_parse(const uint8_t* image, long long nBytes, int numseq, const int* lens, int* nRuns, long long* entries, std::vector<long long>* pairStart);

// ---- the walk's tables (ka_ens.hip kernels, KaEnsCore in ka_ens_core.h): a batch of families with the same number of members;
// one family is a batch of one ----
// Sequences and residues are numbered flat over the batch; a table named first...[nFam + 1] ascends and is searched for the
// family of a flat index.  The residues a candidate names are numbered inside its family.
struct KaEnsFam {
        int firstSeq, firstRes, N, maxlen;
        int nJC;                   // chunks of KA_ENS_JCHUNK sequences j: the family has N * nJC workgroups in a walk
        int colInLds;              // the member columns of a sequence fit in LDS next to the three per-residue arrays
        int minSup;                // the last consensus: levels n_runs .. minSup
        int pad;
        long long cntFirst;        // the count table of one level: [N][N] entries per family, those of the families before this one
};

struct KaEnsFamArgs {
        int nFam, S, T, R;
        const KaEnsFam* fams;
        const int* firstSeq;       // [nFam + 1]
        const int* blkFirst;       // [nFam + 1] walk workgroups of the families before f
        const int* offs;           // [S + 1] first residue of flat sequence s
        const int* lens;           // [S]
        const int* col;            // [R][T]
        const int16_t* res;        // member k at resBase[k]; in it family f at memCell[k * (nFam + 1) + f]: [N_f][memW[k * nFam + f]]
        long long resBase[KA_ENS_MAX_RUNS];
        const int* memCell;
        const int* memW;
        // the alignments X of SCORE / CONF, one per family: their own tables (or those of a member)
        const int* colX;           // [T]
        const int16_t* resX;       // family f at xCell[f]: [N_f][xW[f]]
        const int* xCell;          // [nFam + 1]
        const int* xW;             // [nFam]; <= 0: the family is skipped
        const int* xCol;           // [nFam + 1] CONF: columns of the families before f
        int blk0;                  // first workgroup of this launch (COUNT: of the counted rows; WRITE: of the chunk)
        int level;                 // WRITE: support value of the candidates
        // the count table of a launch holds the flat rows row0 .. row0 + rows alone: level n_runs - lv at lv * E, its rows at lv * rows
        int row0, rows;
        long long E, cnt0;         // entries of one level; the entry (cntFirst + il * N) of row0 in a table of all rows
        unsigned long long* score; // SCORE: [nFam]
        int* supSum;               // CONF: [T]
        int* nPair;                // CONF: [T]
        int* cnt;                  // COUNT: candidates per (level, family, i, j)
        const long long* pairOff;  // WRITE: the same entries scanned along j
        const long long* rowBase;  // WRITE: first slot of row (level, flat i), relative to its chunk
        int2* out;                 // WRITE: (residue of i, residue of j), numbered inside the family
};

// ka_ens.hip
void ka_ens_launch_walk(int mode, const KaEnsFamArgs& a, int nBlocks, size_t lds, hipStream_t s);
void ka_ens_launch_row_scan(const KaEnsFamArgs& a, int nRows, long long* pairOff, long long* rowTot, hipStream_t s);   // nRows = levels * a.rows
void ka_ens_launch_conf(const KaEnsFamArgs& a, int cells, int cols, float* conf, float* colConf, hipStream_t s);
