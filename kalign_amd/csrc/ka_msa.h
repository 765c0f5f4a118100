// ka_msa.h -- the rows of a finished alignment and their two position maps (ka_msa.hip), for every stage that reads
// finished rows (ka_ens.*, ka_cmp.*):
//     col[offs[s] + r]        the column of residue r of sequence s
//     res[s * resStride + c]  the residue of s at column c, or -1
// Includes hip_runtime.h, stdint.h and <vector> only: an edit here does not recompile the task kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

// a residue is an ASCII letter (isalpha in the C locale; pos_matrix_from_msa, poar.c:143-174); every other byte is a gap
__host__ __device__ inline bool ka_msa_is_residue(unsigned b) { return (b | 32u) - 'a' < 26u; }

__device__ __forceinline__ long long ka_msa_wave_sum(long long v)
{
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        return v;
}

// the last f in [0, n) with first[f] <= x (first ascends, first[0] <= x; equal neighbours are empty ranges and are
// skipped): how a wave or workgroup of a batched kernel finds the family (or job) of its flat index -- wave-uniform, a
// dozen scalar loads for thousands of families
__device__ __forceinline__ int ka_fam_find(const int* first, int n, int x)
{
        int lo = 0, hi = n - 1;
        while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (first[mid] <= x) lo = mid;
                else hi = mid - 1;
        }
        return lo;
}

// one row of W bytes -> both maps, by the 64 lanes of one wave: rs[c] for every c below resStride (-1 at gaps and from W
// on), cs[r] = c for every residue, the residue rank of a column from a ballot prefix.  A step's bytes are loaded one step
// ahead: the rank chain never waits for memory.  The host has checked the row's letter count against len; the rank guard
// keeps the writes in place regardless.
__device__ __forceinline__ void ka_msa_map_row(const uint8_t* row, int W, int resStride, int len, int* cs, int16_t* rs, int lane)
{
        const unsigned long long below = (1ull << lane) - 1ull;
        int run = 0;
        unsigned b = lane < W ? row[lane] : 0u;                  // (0 is no letter)
        for (int cb = 0; cb < resStride; cb += 64) {
                const int c = cb + lane;
                const unsigned next = c + 64 < W ? row[c + 64] : 0u;
                const bool isr = ka_msa_is_residue(b);
                const unsigned long long m = __ballot(isr);
                const int r = run + __popcll(m & below);
                const bool put = isr && r < len;
                if (c < resStride) rs[c] = put ? (int16_t)r : (int16_t)-1;
                if (put) cs[r] = c;
                run += __popcll(m);
                b = next;
        }
}

// the sequences whose rows the alignments hold: lengths and flat residue numbering, on the host
struct KaSeqSet {
        int N = 0, T = 0, maxlen = 0;          // sequences, residues, longest sequence
        std::vector<int> lens, offs;           // offs[s]: first residue of sequence s in the flat numbering, offs[N] = T

        // checks the lengths (none negative, none above max_res -- `why` ends that message --, fewer than 2^31 residues
        // in all) and numbers the residues; errors read "<who>: ..."
        int set(const char* who, int numseq, const int* lens, int max_res, const char* why);
};

// rows of an alignment of the set: alnlen columns fit the stride, row s holds lens[s] letters
int ka_msa_check_rows(const char* who, const KaSeqSet& q, const uint8_t* rows, long long stride, int alnlen);
// the rows to N x alnlen bytes at dst, stream-ordered
int ka_msa_upload_rows(const KaSeqSet& q, uint8_t* dst, const uint8_t* rows, long long stride, int alnlen, hipStream_t s);
// both maps of the device rows of a batch of families whose S sequences are numbered flat (device tables; one alignment is a
// batch of one): the rows of family f at rowOff[f], W[f] + rowPad bytes apart (W[f] <= 0: none), its res rows W[f] entries
// each from res + cell[f], -1 at gaps
struct KaMsaFamRows { int nFam, S; const int* firstSeq; const int* offs; const int* lens; };
void ka_msa_launch_maps_fam(const KaMsaFamRows& t, const uint8_t* rows, const long long* rowOff, const int* W, const int* cell, int rowPad, int* col,
                            int16_t* res, hipStream_t s);
