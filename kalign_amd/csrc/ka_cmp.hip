// ka_cmp.hip -- an alignment scored against a reference alignment on the device (kalign_msa_compare,
// kalign_msa_compare_detailed, kalign_msa_compare_with_mask; lib/src/msa_cmp.c).
//
// The reference walks every unordered pair of rows of both alignments and counts, per residue, whether its partner in
// the other sequence agrees.  With col[i][ri] the column of residue ri of sequence i and res[j][c] the residue of j at
// column c (or -1), every counter is a sum over ordered pairs (i -> j, i != j) and residues ri of i of an indicator of
//     pR = resR[j][colR[i][ri]]   and   pT = resT[j][colT[i][ri]]
// (ka_cmp.h lists them).  All are exact integer counts, so the device reproduces the reference bit for bit.
//
//   cmp_col_count  a wave per reference column: its residues (the column mask's gap fraction, TC's "two residues")
//   cmp_mask       the column mask: the reference's float rule on the gap fraction, or the caller's array
//   cmp_walk       the pair walk: a workgroup takes tiles of KA_CMP_TI sequences i x TJ sequences j; the tile's res rows
//                  of both alignments are staged in LDS, each lane takes a residue of the tile's i rows (its two columns
//                  and scored bit in registers) and gathers its partners in every j from LDS
//   cmp_reduce     the workgroups' slabs summed per test
//   cmp_tc         a wave per scored reference column with two residues or more: do they all sit in one test column?
// The position maps themselves are built by ka_msa.hip, the res rows padded to ka_cmp_pad entries.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <algorithm>
#include "ka_cmp.h"
#include "ka_msa.h"

#define CMP_THREADS 256
#define CMP_WAVES (CMP_THREADS / 64)

__global__ __launch_bounds__(CMP_THREADS) void cmp_col_count(const int16_t* res, int W, int Wp, int N, int* colCnt)
{
        const int lane = threadIdx.x & 63;
        for (int c = blockIdx.x * CMP_WAVES + (threadIdx.x >> 6); c < W; c += gridDim.x * CMP_WAVES) {
                long long n = 0;
                for (int s = lane; s < N; s += 64) n += res[(long long)s * Wp + c] >= 0;
                n = ka_msa_wave_sum(n);
                if (lane == 0) colCnt[c] = (int)n;
        }
}

// kalign_msa_compare_detailed: every column when max_gap_frac < 0, else (float)ngaps / (float)numseq <= max_gap_frac
// (IEEE float division: the build has no fast-math); kalign_msa_compare_with_mask: mask[c] != 0
__global__ void cmp_mask(const int* colCnt, int W, int N, float maxGapFrac, const int* mask, uint8_t* scored)
{
        const int c = blockIdx.x * blockDim.x + threadIdx.x;
        if (c >= W) return;
        int v;
        if (mask) v = mask[c] != 0;
        else if (maxGapFrac < 0.0f) v = 1;
        else v = (float)(N - colCnt[c]) / (float)N <= maxGapFrac;
        scored[c] = (uint8_t)v;
}

__global__ __launch_bounds__(CMP_THREADS) void cmp_walk(KaCmpArgs a)
{
        extern __shared__ uint4 cmp_lds[];
        __shared__ long long wsum[CMP_WAVES][KA_CMP_WALK];
        const int k = blockIdx.y;
        const int WRp = a.WRp, WTp = a.tWp[k];
        const int* colT = a.colT + (long long)k * a.T;
        const int16_t* resT = a.resT + a.tResOff[k];
        int16_t* rL = (int16_t*)cmp_lds;                         // [TJ][WRp]
        int16_t* tL = rL + a.TJ * WRp;                           // [TJ][WTp]
        long long acc[KA_CMP_WALK] = {};
        const int nTiles = a.nTI * a.nTJ;
        for (int tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
                const int i0 = (tile / a.nTJ) * KA_CMP_TI, j0 = (tile % a.nTJ) * a.TJ;
                const int i1 = min(a.N, i0 + KA_CMP_TI), nj = min(a.N, j0 + a.TJ) - j0;
                __syncthreads();                                 // the last tile's gathers are done
                {
                        // rows j0 .. j0 + nj - 1 lie back to back in both maps, 16-byte aligned (padded strides)
                        const uint4* src = (const uint4*)(a.resR + (long long)j0 * WRp);
                        uint4* dst = (uint4*)rL;
                        for (int t = threadIdx.x; t < nj * WRp / 8; t += CMP_THREADS) dst[t] = src[t];
                        src = (const uint4*)(resT + (long long)j0 * WTp);
                        dst = (uint4*)tL;
                        for (int t = threadIdx.x; t < nj * WTp / 8; t += CMP_THREADS) dst[t] = src[t];
                }
                __syncthreads();
                const int e1 = a.offs[i1];
                for (int e = a.offs[i0] + threadIdx.x; e < e1; e += CMP_THREADS) {
                        const int cr = a.colR[e], ct = colT[e];
                        const int sc = a.scored[cr];
                        int ra = 0, ta = 0, ia = 0, ig = 0;
#pragma unroll 4
                        for (int jj = 0; jj < nj; jj++) {
                                const int pR = rL[jj * WRp + cr], pT = tL[jj * WTp + ct];
                                ra += pR >= 0;
                                ta += pT >= 0;
                                ia += pR >= 0 && pR == pT;
                                ig += (pR & pT) < 0;
                        }
                        // i itself among the tile's j: its own residue is its partner in both (pR == pT == ri)
                        const int self = (unsigned)(a.seqOf[e] - j0) < (unsigned)nj;
                        ra -= self; ta -= self; ia -= self;
                        acc[KA_CMP_REF_ALIGNED] += ra;
                        acc[KA_CMP_TEST_ALIGNED] += ta;
                        acc[KA_CMP_IDENT_ALIGNED] += ia;
                        acc[KA_CMP_IDENT_GAPS] += ig;
                        // the scored bit belongs to the residue's reference column, the same for every j
                        acc[KA_CMP_REF_SCORED] += sc ? ra : 0;
                        acc[KA_CMP_COMMON_SCORED] += sc ? ia : 0;
                }
        }
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
        for (int q = 0; q < KA_CMP_WALK; q++) {
                const long long t = ka_msa_wave_sum(acc[q]);
                if (lane == 0) wsum[wave][q] = t;
        }
        __syncthreads();
        if (threadIdx.x < KA_CMP_WALK) {
                long long t = 0;
                for (int w = 0; w < CMP_WAVES; w++) t += wsum[w][threadIdx.x];
                a.slab[((long long)k * gridDim.x + blockIdx.x) * KA_CMP_WALK + threadIdx.x] = t;
        }
}

// one workgroup per test: the walk's slabs summed in a fixed order
__global__ __launch_bounds__(CMP_THREADS) void cmp_reduce(const long long* slab, int gridX, long long* sums)
{
        __shared__ long long wsum[CMP_WAVES][KA_CMP_WALK];
        const int k = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        long long acc[KA_CMP_WALK] = {};
        for (int g = threadIdx.x; g < gridX; g += CMP_THREADS)
#pragma unroll
                for (int q = 0; q < KA_CMP_WALK; q++) acc[q] += slab[((long long)k * gridX + g) * KA_CMP_WALK + q];
#pragma unroll
        for (int q = 0; q < KA_CMP_WALK; q++) {
                const long long t = ka_msa_wave_sum(acc[q]);
                if (lane == 0) wsum[wave][q] = t;
        }
        __syncthreads();
        if (threadIdx.x < KA_CMP_WALK) {
                long long t = 0;
                for (int w = 0; w < CMP_WAVES; w++) t += wsum[w][threadIdx.x];
                sums[(long long)k * KA_CMP_WALK + threadIdx.x] = t;
        }
}

// TC (compare_with_mask_helper): a scored reference column with >= 2 residues counts; it is correct when every one of
// its residues sits in one test column
__global__ __launch_bounds__(CMP_THREADS) void cmp_tc(KaCmpArgs a)
{
        const int k = blockIdx.y, lane = threadIdx.x & 63;
        const int* colT = a.colT + (long long)k * a.T;
        unsigned long long correct = 0, total = 0;
        for (int c = blockIdx.x * CMP_WAVES + (threadIdx.x >> 6); c < a.WR; c += gridDim.x * CMP_WAVES) {
                if (!a.scored[c] || a.colCnt[c] < 2) continue;   // (wave-uniform)
                int lo = INT_MAX, hi = INT_MIN;
                for (int s = lane; s < a.N; s += 64) {
                        const int r = a.resR[(long long)s * a.WRp + c];
                        if (r >= 0) {
                                const int t = colT[a.offs[s] + r];
                                lo = min(lo, t);
                                hi = max(hi, t);
                        }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                        lo = min(lo, __shfl_xor(lo, o, 64));
                        hi = max(hi, __shfl_xor(hi, o, 64));
                }
                total++;
                correct += lo == hi;
        }
        if (lane == 0 && total) {
                atomicAdd(&a.tc[2 * k], correct);
                atomicAdd(&a.tc[2 * k + 1], total);
        }
}

void ka_cmp_launch_col_count(const int16_t* res, int W, int Wp, int N, int* colCnt, hipStream_t s)
{
        const int blocks = std::min((W + CMP_WAVES - 1) / CMP_WAVES, 2048);
        cmp_col_count<<<blocks, CMP_THREADS, 0, s>>>(res, W, Wp, N, colCnt);
}

void ka_cmp_launch_mask(const int* colCnt, int W, int N, float maxGapFrac, const int* mask, uint8_t* scored, hipStream_t s)
{
        cmp_mask<<<(W + 255) / 256, 256, 0, s>>>(colCnt, W, N, maxGapFrac, mask, scored);
}

int ka_cmp_launch_walk(const KaCmpArgs& a, int K, int gridX, size_t lds, hipStream_t s)
{
        if (lds > 65536 && hipFuncSetAttribute((const void*)cmp_walk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return 1;
        cmp_walk<<<dim3(gridX, K), CMP_THREADS, lds, s>>>(a);
        cmp_reduce<<<K, CMP_THREADS, 0, s>>>(a.slab, gridX, a.sums);
        return 0;
}

void ka_cmp_launch_tc(const KaCmpArgs& a, int K, hipStream_t s)
{
        const int blocks = std::min((a.WR + CMP_WAVES - 1) / CMP_WAVES, 512);
        cmp_tc<<<dim3(blocks, K), CMP_THREADS, 0, s>>>(a);
}
