// ka_cmp_fam.hip -- a batch of families scored against their reference alignments: the kernels of ka_cmp.hip in the form
// that takes every family of the batch in one launch (ka_cmp_fam.cpp is the host side, ka_cmp.h the shared tables).
//
// Sequences, residues and reference columns are numbered flat over the batch.  A wave or workgroup finds the family of
// its flat index by a search of an ascending first-index table (cmpf_find: wave-uniform, a dozen scalar loads for
// thousands of families), then works with that family's geometry from its KaCmpFam.
//
//   cmpf_maps       a wave per row of the packed rows: msa_maps' ballot-prefix rank with the row's own start, width and
//                   res stride
//   cmpf_col_count  a wave per flat reference column: its residues
//   cmpf_mask       a thread per flat reference column: the family's mask, or the float rule with the family's N and fraction
//   cmpf_walk       workgroups stride over the tiles (family, i-tile, j-tile) of one LDS class; a tile is a tile of cmp_walk.
//                   Its counters fit an int; they are summed per wave, then per workgroup, and added to the family's sums
//                   with 64-bit vector atomics (exact integers: the order of the additions does not matter)
//   cmpf_tc         a wave per KA_CMPF_TCCHUNK consecutive flat reference columns, its counts added per family
#include <hip/hip_runtime.h>
#include <limits.h>
#include <algorithm>
#include "ka_cmp.h"
#include "ka_msa.h"

#define CMPF_THREADS 256
#define CMPF_WAVES (CMPF_THREADS / 64)

// the last f in [0, n) with first[f] <= x (first ascends, first[0] <= x; equal neighbours are empty ranges and are skipped)
__device__ __forceinline__ int cmpf_find(const int* first, int n, int x)
{
        int lo = 0, hi = n - 1;
        while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (first[mid] <= x) lo = mid;
                else hi = mid - 1;
        }
        return lo;
}

__global__ __launch_bounds__(CMPF_THREADS) void cmpf_maps(KaCmpFamArgs a, int test)
{
        const int s = blockIdx.x * CMPF_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (s >= a.S) return;
        const KaCmpFam& d = a.fams[cmpf_find(a.firstSeq, a.nFam, s)];
        const KaCmpSide& sd = test ? d.t : d.r;
        const int W = sd.W, Wp = sd.Wp, loc = s - d.firstSeq;
        const uint8_t* row = a.rows + sd.rowOff + (long long)loc * (W + 1);
        int16_t* rs = (test ? a.resT : a.resR) + sd.resOff + (long long)loc * Wp;
        int* cs = (test ? a.colT : a.colR) + a.offs[s];
        const int len = a.lens[s];
        const unsigned long long below = (1ull << lane) - 1ull;
        int run = 0;
        for (int cb = 0; cb < Wp; cb += 64) {
                const int c = cb + lane;
                const bool isr = c < W && ka_msa_is_residue(row[c]);
                const unsigned long long m = __ballot(isr);
                const int r = run + __popcll(m & below);
                const bool put = isr && r < len;
                if (c < Wp) rs[c] = put ? (int16_t)r : (int16_t)-1;
                if (put) cs[r] = c;
                run += __popcll(m);
        }
}

__global__ __launch_bounds__(CMPF_THREADS) void cmpf_col_count(KaCmpFamArgs a)
{
        const int lane = threadIdx.x & 63;
        for (long long cc = (long long)blockIdx.x * CMPF_WAVES + (threadIdx.x >> 6); cc < a.cols; cc += (long long)gridDim.x * CMPF_WAVES) {
                const int c = (int)cc;
                const KaCmpFam& d = a.fams[cmpf_find(a.firstCol, a.nFam, c)];
                const int16_t* res = a.resR + d.r.resOff + (c - d.firstCol);
                int n = 0;
                for (int s = lane; s < d.N; s += 64) n += res[(long long)s * d.r.Wp] >= 0;
                n = (int)ka_msa_wave_sum(n);
                if (lane == 0) a.colCnt[c] = n;
        }
}

// cmp_mask's rules with the family's N, fraction and mask
__global__ void cmpf_mask(KaCmpFamArgs a)
{
        const long long cc = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (cc >= a.cols) return;
        const int c = (int)cc, f = cmpf_find(a.firstCol, a.nFam, c);
        const int N = a.fams[f].N;
        const long long mo = a.maskOff ? a.maskOff[f] : -1;
        const float frac = a.frac ? a.frac[f] : -1.0f;
        int v;
        if (mo >= 0) v = a.masks[mo + (c - a.fams[f].firstCol)] != 0;
        else if (frac < 0.0f) v = 1;
        else v = (float)(N - a.colCnt[c]) / (float)N <= frac;
        a.scored[c] = (uint8_t)v;
}

__global__ __launch_bounds__(CMPF_THREADS) void cmpf_walk(KaCmpFamArgs a, const int* first, int nTiles)
{
        extern __shared__ uint4 cmpf_lds[];
        __shared__ int wsum[CMPF_WAVES][KA_CMP_WALK];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
                const int f = cmpf_find(first, a.nFam, tile);
                const KaCmpFam& d = a.fams[f];
                const int N = d.N, TJ = d.TJ, WRp = d.r.Wp, WTp = d.t.Wp;
                const int t = tile - first[f];
                const int i0 = (t / d.nTJ) * KA_CMP_TI, j0 = (t % d.nTJ) * TJ;
                const int i1 = min(N, i0 + KA_CMP_TI), nj = min(N, j0 + TJ) - j0;
                int16_t* rL = (int16_t*)cmpf_lds;                // [TJ][WRp]
                int16_t* tL = rL + TJ * WRp;                     // [TJ][WTp]
                __syncthreads();                                 // the last tile's gathers and its sums are done
                {
                        // rows j0 .. j0 + nj - 1 lie back to back in both maps, 16-byte aligned (padded strides, and every
                        // family's map a multiple of them)
                        const uint4* src = (const uint4*)(a.resR + d.r.resOff + (long long)j0 * WRp);
                        uint4* dst = (uint4*)rL;
                        for (int q = threadIdx.x; q < nj * WRp / 8; q += CMPF_THREADS) dst[q] = src[q];
                        src = (const uint4*)(a.resT + d.t.resOff + (long long)j0 * WTp);
                        dst = (uint4*)tL;
                        for (int q = threadIdx.x; q < nj * WTp / 8; q += CMPF_THREADS) dst[q] = src[q];
                }
                __syncthreads();
                const uint8_t* scored = a.scored + d.firstCol;
                // a lane's share of a tile: at most 16 * 32767 / 256 residues x 32 partners -- an int holds a workgroup's sum
                int acc[KA_CMP_WALK] = {};
                const int e1 = a.offs[d.firstSeq + i1];
                for (int e = a.offs[d.firstSeq + i0] + threadIdx.x; e < e1; e += CMPF_THREADS) {
                        const int cr = a.colR[e], ct = a.colT[e];
                        const int sc = scored[cr];
                        int ra = 0, ta = 0, ia = 0, ig = 0;
#pragma unroll 4
                        for (int jj = 0; jj < nj; jj++) {
                                const int pR = rL[jj * WRp + cr], pT = tL[jj * WTp + ct];
                                ra += pR >= 0;
                                ta += pT >= 0;
                                ia += pR >= 0 && pR == pT;
                                ig += (pR & pT) < 0;
                        }
                        // i itself among the tile's j (indices inside the family): its own residue is its partner in both
                        const int self = (unsigned)(a.seqOf[e] - j0) < (unsigned)nj;
                        ra -= self; ta -= self; ia -= self;
                        acc[KA_CMP_REF_ALIGNED] += ra;
                        acc[KA_CMP_TEST_ALIGNED] += ta;
                        acc[KA_CMP_IDENT_ALIGNED] += ia;
                        acc[KA_CMP_IDENT_GAPS] += ig;
                        acc[KA_CMP_REF_SCORED] += sc ? ra : 0;
                        acc[KA_CMP_COMMON_SCORED] += sc ? ia : 0;
                }
#pragma unroll
                for (int q = 0; q < KA_CMP_WALK; q++) {
                        int v = acc[q];
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
                        if (lane == 0) wsum[wave][q] = v;
                }
                __syncthreads();
                if (threadIdx.x < KA_CMP_WALK) {
                        long long v = 0;
                        for (int w = 0; w < CMPF_WAVES; w++) v += wsum[w][threadIdx.x];
                        if (v) atomicAdd(&a.sums[(long long)f * KA_CMPF_SUMS + threadIdx.x], (unsigned long long)v);
                }
        }
}

// cmp_tc over the flat reference columns: a wave takes KA_CMPF_TCCHUNK consecutive columns and hands its counts over
// whenever the family changes
__global__ __launch_bounds__(CMPF_THREADS) void cmpf_tc(KaCmpFamArgs a)
{
        const int lane = threadIdx.x & 63;
        const long long c0 = ((long long)blockIdx.x * CMPF_WAVES + (threadIdx.x >> 6)) * KA_CMPF_TCCHUNK;
        if (c0 >= a.cols) return;
        const int c1 = (int)min((long long)a.cols, c0 + KA_CMPF_TCCHUNK);
        int f = cmpf_find(a.firstCol, a.nFam, (int)c0);
        unsigned long long correct = 0, total = 0;
        for (int c = (int)c0; c < c1; c++) {
                if (c >= a.firstCol[f + 1]) {
                        if (lane == 0 && total) {
                                atomicAdd(&a.sums[(long long)f * KA_CMPF_SUMS + KA_CMP_WALK], correct);
                                atomicAdd(&a.sums[(long long)f * KA_CMPF_SUMS + KA_CMP_WALK + 1], total);
                        }
                        correct = total = 0;
                        while (c >= a.firstCol[f + 1]) f++;      // (c < cols = firstCol[nFam]: f stays below nFam)
                }
                if (!a.scored[c] || a.colCnt[c] < 2) continue;   // (wave-uniform)
                const KaCmpFam& d = a.fams[f];
                const int16_t* res = a.resR + d.r.resOff + (c - d.firstCol);
                const int* colT = a.colT;
                int lo = INT_MAX, hi = INT_MIN;
                for (int s = lane; s < d.N; s += 64) {
                        const int r = res[(long long)s * d.r.Wp];
                        if (r >= 0) {
                                const int t = colT[a.offs[d.firstSeq + s] + r];
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
                atomicAdd(&a.sums[(long long)f * KA_CMPF_SUMS + KA_CMP_WALK], correct);
                atomicAdd(&a.sums[(long long)f * KA_CMPF_SUMS + KA_CMP_WALK + 1], total);
        }
}

void ka_cmpf_launch_maps(const KaCmpFamArgs& a, int test, hipStream_t s)
{
        cmpf_maps<<<(a.S + CMPF_WAVES - 1) / CMPF_WAVES, CMPF_THREADS, 0, s>>>(a, test);
}

void ka_cmpf_launch_col_count(const KaCmpFamArgs& a, hipStream_t s)
{
        const int blocks = (int)std::min<long long>(((long long)a.cols + CMPF_WAVES - 1) / CMPF_WAVES, 4096);
        cmpf_col_count<<<blocks, CMPF_THREADS, 0, s>>>(a);
}

void ka_cmpf_launch_mask(const KaCmpFamArgs& a, hipStream_t s)
{
        cmpf_mask<<<(unsigned)(((long long)a.cols + 255) / 256), 256, 0, s>>>(a);
}

int ka_cmpf_launch_walk(const KaCmpFamArgs& a, const int* first, int nTiles, size_t lds, hipStream_t s)
{
        if (lds > 65536 && hipFuncSetAttribute((const void*)cmpf_walk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return 1;
        cmpf_walk<<<std::min(nTiles, KA_CMPF_GRID), CMPF_THREADS, lds, s>>>(a, first, nTiles);
        return 0;
}

void ka_cmpf_launch_tc(const KaCmpFamArgs& a, hipStream_t s)
{
        const int perBlock = CMPF_WAVES * KA_CMPF_TCCHUNK;
        cmpf_tc<<<(unsigned)(((long long)a.cols + perBlock - 1) / perBlock), CMPF_THREADS, 0, s>>>(a);
}
