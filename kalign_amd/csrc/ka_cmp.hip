// ka_cmp.hip -- alignments scored against reference alignments on the device (kalign_msa_compare,
// kalign_msa_compare_detailed, kalign_msa_compare_with_mask; lib/src/msa_cmp.c): the one set of kernels behind ka_cmp
// (K tests of one reference) and ka_cmp_fam (one test per family), over the job table of ka_cmp.h.
//
// The reference walks every unordered pair of rows of both alignments and counts, per residue, whether its partner in
// the other sequence agrees.  With col[i][ri] the column of residue ri of sequence i and res[j][c] the residue of j at
// column c (or -1), every counter is a sum over ordered pairs (i -> j, i != j) and residues ri of i of an indicator of
//     pR = resR[j][colR[i][ri]]   and   pT = resT[j][colT[i][ri]]
// (ka_cmp.h lists them).  All are exact integer counts, so the device reproduces the reference bit for bit, and neither
// the tiling nor the order of the additions can show in a result.
//
//   cmp_maps       a wave per row of the uploaded rows (the references', or the jobs' test rows): ka_msa_map_row with the
//                  row's own start, stride, width and res stride
//   cmp_col_count  a wave per reference column: its residues (the column mask's gap fraction, TC's "two residues")
//   cmp_mask       a thread per reference column: the reference's mask, or the float rule with its N and fraction
//   cmp_walk       the pair walk: workgroups stride over the tiles (job, KA_CMP_TI sequences i, TJ sequences j) of one LDS
//                  class.  The tile's res rows of both alignments are staged in LDS, each lane takes a residue of the
//                  tile's i rows (its two columns and scored bit in registers) and gathers its partners in every j from
//                  LDS.  A tile's counters fit an int; a lane carries them in 64 bits over its workgroup's consecutive
//                  tiles of one job and the workgroup hands them over -- wave sums, then 64-bit vector atomics on the
//                  job's sums -- when the job changes and at the end
//   cmp_tc         a wave per chunk of consecutive job columns: a scored reference column with two residues or more -- do
//                  they all sit in one test column?  Its counts are handed over in the same way
//   cmp_walk_detail  the walk's body once more (cmp_walk_body<true>): every lane also adds its residue's ra / ta / ia to the
//                  three planes of detRes -- the counts behind a per-residue ground truth (ka_cmp_fam_detail)
//   cmp_cols       a wave per chunk of consecutive test columns or reference columns: the residues of the column, the sum
//                  of their plane-2 counts, and whether they all sit in one column of the other alignment
#include <hip/hip_runtime.h>
#include <limits.h>
#include <algorithm>
#include "ka_cmp.h"
#include "ka_msa.h"

#define CMP_THREADS 256
#define CMP_WAVES (CMP_THREADS / 64)

__global__ __launch_bounds__(CMP_THREADS) void cmp_maps(KaCmpTab a, int test)
{
        const int x = blockIdx.x * CMP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (x >= (test ? a.jobRows : a.S)) return;
        const int* first = test ? a.jobRow : a.refSeq;
        const int f = ka_fam_find(first, test ? a.nJob : a.nRef, x);
        const KaCmpJob& d = (test ? a.jobs : a.refs)[f];
        const KaCmpSide& sd = test ? d.t : d.r;
        const int loc = x - first[f], s = d.firstSeq + loc;
        int* cs = test ? a.colT + d.colOff + a.offs[s] : a.colR + a.offs[s];
        int16_t* rs = (test ? a.resT : a.resR) + sd.resOff + (long long)loc * sd.Wp;
        ka_msa_map_row(a.rows + sd.rowOff + loc * sd.stride, sd.W, sd.Wp, a.lens[s], cs, rs, lane);
}

__global__ __launch_bounds__(CMP_THREADS) void cmp_col_count(KaCmpTab a)
{
        const int lane = threadIdx.x & 63;
        for (long long cc = (long long)blockIdx.x * CMP_WAVES + (threadIdx.x >> 6); cc < a.cols; cc += (long long)gridDim.x * CMP_WAVES) {
                const int c = (int)cc;
                const KaCmpJob& d = a.refs[ka_fam_find(a.refCol, a.nRef, c)];
                const int16_t* res = a.resR + d.r.resOff + (c - d.firstCol);
                int n = 0;
                for (int s = lane; s < d.N; s += 64) n += res[(long long)s * d.r.Wp] >= 0;
                n = (int)ka_msa_wave_sum(n);
                if (lane == 0) a.colCnt[c] = n;
        }
}

// kalign_msa_compare_detailed: every column when max_gap_frac < 0, else (float)ngaps / (float)numseq <= max_gap_frac
// (IEEE float division: the build has no fast-math); kalign_msa_compare_with_mask: mask[c] != 0
__global__ void cmp_mask(KaCmpTab a)
{
        const long long cc = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (cc >= a.cols) return;
        const int c = (int)cc, f = ka_fam_find(a.refCol, a.nRef, c);
        const int N = a.refs[f].N;
        const long long mo = a.maskOff ? a.maskOff[f] : -1;
        const float frac = a.frac ? a.frac[f] : -1.0f;
        int v;
        if (mo >= 0) v = a.masks[mo + (c - a.refs[f].firstCol)] != 0;
        else if (frac < 0.0f) v = 1;
        else v = (float)(N - a.colCnt[c]) / (float)N <= frac;
        a.scored[c] = (uint8_t)v;
}

// the walk's body in its two forms: DETAIL false is the score call's, DETAIL true also hands out every residue's counts
template <bool DETAIL>
__device__ __forceinline__ void cmp_walk_body(const KaCmpTab& a, const int* first, int nTiles)
{
        extern __shared__ uint4 cmp_lds[];
        __shared__ long long wsum[CMP_WAVES][KA_CMP_WALK];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        long long carry[KA_CMP_WALK] = {};                       // the counters of job `cur` not yet handed over
        int cur = -1;
        for (int tile = blockIdx.x; ; tile += gridDim.x) {
                const int f = tile < nTiles ? ka_fam_find(first, a.nJob, tile) : -1;   // (uniform over the workgroup)
                if (f != cur && cur >= 0) {
#pragma unroll
                        for (int q = 0; q < KA_CMP_WALK; q++) {
                                const long long v = ka_msa_wave_sum(carry[q]);
                                if (lane == 0) wsum[wave][q] = v;
                                carry[q] = 0;
                        }
                        __syncthreads();                         // (the tile body's barriers stand between two hand-overs)
                        if (threadIdx.x < KA_CMP_WALK) {
                                long long v = 0;
                                for (int w = 0; w < CMP_WAVES; w++) v += wsum[w][threadIdx.x];
                                if (v) atomicAdd(&a.sums[(long long)cur * KA_CMP_SUMS + threadIdx.x], (unsigned long long)v);
                        }
                }
                if (f < 0) break;
                cur = f;
                const KaCmpJob d = a.jobs[f];                    // (by value: read once, ahead of the barriers)
                const int N = d.N, TJ = d.TJ, WRp = d.r.Wp, WTp = d.t.Wp;
                const int t = tile - first[f];
                const int i0 = (t / d.nTJ) * KA_CMP_TI, j0 = (t % d.nTJ) * TJ;
                const int i1 = min(N, i0 + KA_CMP_TI), nj = min(N, j0 + TJ) - j0;
                int16_t* rL = (int16_t*)cmp_lds;                 // [TJ][WRp]
                int16_t* tL = rL + TJ * WRp;                     // [TJ][WTp]
                __syncthreads();                                 // the last tile's gathers are done
                {
                        // rows j0 .. j0 + nj - 1 lie back to back in both maps, 16-byte aligned (padded strides, and every
                        // map a multiple of them)
                        const uint4* src = (const uint4*)(a.resR + d.r.resOff + (long long)j0 * WRp);
                        uint4* dst = (uint4*)rL;
                        for (int q = threadIdx.x; q < nj * WRp / 8; q += CMP_THREADS) dst[q] = src[q];
                        src = (const uint4*)(a.resT + d.t.resOff + (long long)j0 * WTp);
                        dst = (uint4*)tL;
                        for (int q = threadIdx.x; q < nj * WTp / 8; q += CMP_THREADS) dst[q] = src[q];
                }
                __syncthreads();
                const uint8_t* scored = a.scored + d.firstCol;
                const int* colT = a.colT + d.colOff;
                // a lane's share of a tile: at most 16 * 32767 / 256 residues x 32 partners -- an int holds it
                int acc[KA_CMP_WALK] = {};
                const int e1 = a.offs[d.firstSeq + i1];
                for (int e = a.offs[d.firstSeq + i0] + threadIdx.x; e < e1; e += CMP_THREADS) {
                        const int cr = a.colR[e], ct = colT[e];
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
                        // i itself among the tile's j (indices inside the reference): its own residue is its partner in
                        // both (pR == pT == ri)
                        const int self = (unsigned)(a.seqOf[e] - j0) < (unsigned)nj;
                        ra -= self; ta -= self; ia -= self;
                        if (DETAIL) {
                                // the residue's counts of this j-tile: nTJ workgroups add to one entry, a wave's lanes to
                                // consecutive ones (256 contiguous bytes per plane); integer adds, so no order shows
                                atomicAdd(a.detRes + e, ra);
                                atomicAdd(a.detRes + (size_t)a.T + e, ta);
                                atomicAdd(a.detRes + 2 * (size_t)a.T + e, ia);
                        }
                        acc[KA_CMP_REF_ALIGNED] += ra;
                        acc[KA_CMP_TEST_ALIGNED] += ta;
                        acc[KA_CMP_IDENT_ALIGNED] += ia;
                        acc[KA_CMP_IDENT_GAPS] += ig;
                        // the scored bit belongs to the residue's reference column, the same for every j
                        acc[KA_CMP_REF_SCORED] += sc ? ra : 0;
                        acc[KA_CMP_COMMON_SCORED] += sc ? ia : 0;
                }
#pragma unroll
                for (int q = 0; q < KA_CMP_WALK; q++) carry[q] += acc[q];
        }
}

__global__ __launch_bounds__(CMP_THREADS) void cmp_walk(KaCmpTab a, const int* first, int nTiles)
{
        cmp_walk_body<false>(a, first, nTiles);
}

__global__ __launch_bounds__(CMP_THREADS) void cmp_walk_detail(KaCmpTab a, const int* first, int nTiles)
{
        cmp_walk_body<true>(a, first, nTiles);
}

// TC (compare_with_mask_helper): a scored reference column with >= 2 residues counts; it is correct when every one of
// its residues sits in one test column.  A wave takes `chunk` consecutive job columns and hands its counts over whenever
// the job changes
__global__ __launch_bounds__(CMP_THREADS) void cmp_tc(KaCmpTab a, int chunk)
{
        const int lane = threadIdx.x & 63;
        const long long c0 = ((long long)blockIdx.x * CMP_WAVES + (threadIdx.x >> 6)) * chunk;
        if (c0 >= a.jobCols) return;
        const int c1 = (int)min((long long)a.jobCols, c0 + chunk);
        int f = ka_fam_find(a.jobCol, a.nJob, (int)c0);
        KaCmpJob d = a.jobs[f];                                  // (by value: its fields stay in registers over the columns)
        int cf = a.jobCol[f], cn = a.jobCol[f + 1];              // the job's columns: cf .. cn - 1
        unsigned long long correct = 0, total = 0;
        for (int c = (int)c0; c < c1; c++) {
                if (c >= cn) {
                        if (lane == 0 && total) {
                                atomicAdd(&a.sums[(long long)f * KA_CMP_SUMS + KA_CMP_WALK], correct);
                                atomicAdd(&a.sums[(long long)f * KA_CMP_SUMS + KA_CMP_WALK + 1], total);
                        }
                        correct = total = 0;
                        while (c >= a.jobCol[f + 1]) f++;        // (c < jobCols = jobCol[nJob]: f stays below nJob)
                        d = a.jobs[f];
                        cf = a.jobCol[f]; cn = a.jobCol[f + 1];
                }
                const int cr = c - cf;                           // the column in the job's reference
                if (!a.scored[d.firstCol + cr] || a.colCnt[d.firstCol + cr] < 2) continue;   // (wave-uniform)
                const int16_t* res = a.resR + d.r.resOff + cr;
                const int* colT = a.colT + d.colOff;
                const int* offs = a.offs + d.firstSeq;
                int lo = INT_MAX, hi = INT_MIN;
                for (int s = lane; s < d.N; s += 64) {
                        const int r = res[(long long)s * d.r.Wp];
                        if (r >= 0) {
                                const int t = colT[offs[s] + r];
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
                atomicAdd(&a.sums[(long long)f * KA_CMP_SUMS + KA_CMP_WALK], correct);
                atomicAdd(&a.sums[(long long)f * KA_CMP_SUMS + KA_CMP_WALK + 1], total);
        }
}

// The column records of a detail call, both sides in one launch.  Side 0: the call's test columns, each against its
// reference -- correct when its residues share one reference column (_column_correctness of the reference's calibration
// benchmark).  Side 1: the references' columns against the tests -- TC's verdict, here for every column.  A wave takes
// `chunk` consecutive columns of one side (waves 0 .. nW0 - 1 serve side 0) and carries the job across them as cmp_tc
// does.  `correct` comes from the columns, `common` from the detailed walk's plane 2: two routes to one fact
// (correct == (common == k (k - 1))).
__global__ __launch_bounds__(CMP_THREADS) void cmp_cols(KaCmpTab a, int chunk, int nW0)
{
        const int lane = threadIdx.x & 63;
        const long long w = (long long)blockIdx.x * CMP_WAVES + (threadIdx.x >> 6);
        const int side = w >= nW0;
        const int* first = side ? a.jobCol : a.tcolFirst;
        const int n = side ? a.jobCols : a.tCols;
        const long long c0 = (w - (side ? nW0 : 0)) * chunk;
        if (c0 >= n) return;
        const int c1 = (int)min((long long)n, c0 + chunk);
        const long long out0 = side ? a.tCols : 0;               // the reference columns' records follow the test columns'
        const int* plane2 = a.detRes + 2 * (size_t)a.T;
        int f = ka_fam_find(first, a.nJob, (int)c0);
        KaCmpJob d = a.jobs[f];                                  // (by value: its fields stay in registers over the columns)
        int cf = first[f], cn = first[f + 1];                    // the job's columns of this side: cf .. cn - 1
        for (int c = (int)c0; c < c1; c++) {
                if (c >= cn) {
                        while (c >= first[f + 1]) f++;           // (c < n = first[nJob]: f stays below nJob)
                        d = a.jobs[f];
                        cf = first[f]; cn = first[f + 1];
                }
                const KaCmpSide& own = side ? d.r : d.t;
                const int16_t* res = (side ? a.resR : a.resT) + own.resOff + (c - cf);
                const int* other = side ? a.colT + d.colOff : a.colR;    // a flat residue's column in the other alignment
                const int* offs = a.offs + d.firstSeq;
                int lo = INT_MAX, hi = INT_MIN;
                long long k = 0, common = 0;
                for (int s = lane; s < d.N; s += 64) {
                        const int r = res[(long long)s * own.Wp];
                        if (r >= 0) {
                                const int e = offs[s] + r;
                                const int t = other[e];
                                lo = min(lo, t);
                                hi = max(hi, t);
                                k++;
                                common += plane2[e];
                        }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                        lo = min(lo, __shfl_xor(lo, o, 64));
                        hi = max(hi, __shfl_xor(hi, o, 64));
                }
                k = ka_msa_wave_sum(k);
                common = ka_msa_wave_sum(common);
                if (lane == 0) {
                        a.detColRes[out0 + c] = (int)k;
                        a.detColCommon[out0 + c] = common;
                        a.detColCorrect[out0 + c] = (uint8_t)(k <= 1 || lo == hi);
                }
        }
}

void ka_cmp_run_maps(const KaCmpTab& a, int test, hipStream_t s)
{
        cmp_maps<<<((test ? a.jobRows : a.S) + CMP_WAVES - 1) / CMP_WAVES, CMP_THREADS, 0, s>>>(a, test);
}

void ka_cmp_run_col_count(const KaCmpTab& a, hipStream_t s)
{
        const int blocks = (int)std::min<long long>(((long long)a.cols + CMP_WAVES - 1) / CMP_WAVES, 4096);
        cmp_col_count<<<blocks, CMP_THREADS, 0, s>>>(a);
}

void ka_cmp_run_mask(const KaCmpTab& a, hipStream_t s)
{
        cmp_mask<<<(unsigned)(((long long)a.cols + 255) / 256), 256, 0, s>>>(a);
}

int ka_cmp_run_walk(const KaCmpTab& a, const int* first, int nTiles, size_t lds, bool detail, hipStream_t s)
{
        const void* kernel = detail ? (const void*)cmp_walk_detail : (const void*)cmp_walk;
        // (64 KiB without asking, the kernel's static LDS included)
        if (lds > 65536 - 1024 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return 1;
        if (detail) cmp_walk_detail<<<std::min(nTiles, KA_CMP_WALK_WGS), CMP_THREADS, lds, s>>>(a, first, nTiles);
        else cmp_walk<<<std::min(nTiles, KA_CMP_WALK_WGS), CMP_THREADS, lds, s>>>(a, first, nTiles);
        return 0;
}

void ka_cmp_run_tc(const KaCmpTab& a, hipStream_t s)
{
        // as many columns per wave as leave 2048 waves (8 per CU), KA_CMP_TCCHUNK at most: a wave per column for one
        // reference of ordinary width, and never thousands of waves handing over to the two sums of one job
        const int chunk = std::max(1, std::min(KA_CMP_TCCHUNK, (a.jobCols + 2047) / 2048));
        const int perBlock = CMP_WAVES * chunk;
        cmp_tc<<<(unsigned)(((long long)a.jobCols + perBlock - 1) / perBlock), CMP_THREADS, 0, s>>>(a, chunk);
}

void ka_cmp_run_cols(const KaCmpTab& a, hipStream_t s)
{
        // the TC pass's rule over the columns of both sides: 2048 waves or more, KA_CMP_TCCHUNK columns per wave at most
        const long long all = (long long)a.tCols + a.jobCols;
        const int chunk = (int)std::max<long long>(1, std::min<long long>(KA_CMP_TCCHUNK, (all + 2047) / 2048));
        const long long nW0 = ((long long)a.tCols + chunk - 1) / chunk, nW1 = ((long long)a.jobCols + chunk - 1) / chunk;
        if (nW0 + nW1 == 0) return;
        cmp_cols<<<(unsigned)((nW0 + nW1 + CMP_WAVES - 1) / CMP_WAVES), CMP_THREADS, 0, s>>>(a, chunk, (int)nW0);
}
