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

// the sequences whose rows the alignments hold: lengths and flat residue numbering, here and on the device
struct KaSeqSet {
        int N = 0, T = 0, maxlen = 0;          // sequences, residues, longest sequence
        std::vector<int> lens, offs;           // offs[s]: first residue of sequence s in the flat numbering, offs[N] = T
        int* dOffs = nullptr;                  // [N + 1]
        int* dLens = nullptr;                  // [N]

        // checks the lengths (none negative, none above max_res -- `why` ends that message --, fewer than 2^31 residues
        // in all) and numbers the residues, on the host alone; errors read "<who>: ..."
        int set(const char* who, int numseq, const int* lens, int max_res, const char* why);
        // set(), then the lengths copied to the current device
        int init(const char* who, int numseq, const int* lens, int max_res, const char* why);
        void release();
};

// rows of an alignment of the set: alnlen columns fit the stride, row s holds lens[s] letters
int ka_msa_check_rows(const char* who, const KaSeqSet& q, const uint8_t* rows, long long stride, int alnlen);
// the rows to N x alnlen bytes at dst, stream-ordered
int ka_msa_upload_rows(const KaSeqSet& q, uint8_t* dst, const uint8_t* rows, long long stride, int alnlen, hipStream_t s);
// both maps of N x W device rows (row stride rowStride); res gets resStride >= W entries per row, -1 at gaps and from W on
void ka_msa_launch_maps(const uint8_t* rows, int rowStride, int W, int resStride, const KaSeqSet& q, int* col, int16_t* res, hipStream_t s);
