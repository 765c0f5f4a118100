// ka_ens.hip -- the ensemble consensus stage on the device (kalign_ensemble's tail, lib/src/ensemble.c:341-; poar.c,
// consensus_msa.c), for a batch of families in one launch; one family is a batch of one (KaEnsCore, ka_ens_core.h, is the
// host side, ka_ens.h holds the tables).
//
// The reference keeps, for every pair of sequences, a sorted table of the residue pairs (POARs) that some member
// aligns, with a bit per member.  The table is a function of the members' position maps: with col_k[s][r] the column
// of residue r of sequence s in member k and res_k[s][c] the residue of s at column c of member k (or -1),
//     support(i, ri, j, rj) = #{ k : res_k[j][col_k[i][ri]] == rj }  ( = #{ k : col_k[i][ri] == col_k[j][rj] } ).
// So every quantity of the stage is an integer count of n_runs gathers per (i, ri, j):
//   SCORE  sum over the aligned pairs of an alignment X of (support - 1)        (score_alignment_poar, exact int64)
//   CONF   per residue of X: sum of support over its partners, number of partners (compute_residue_confidence)
//   COUNT  per pair (i, j): distinct (ri, rj) per support level                  (build_consensus' candidate list,
//   WRITE  ... and the candidates of one level, in the reference's order          highest level first)
// Sequences and residues are numbered flat over the batch.  A wave or workgroup finds the family of its flat index by a
// search of an ascending first-index table (ka_fam_find, ka_msa.h: wave-uniform), then works with that family's geometry from its
// KaEnsFam and the per-family entries of the member tables.
//
//   (maps)        ka_msa.hip's msa_maps_fam: a wave per row, with the row's own start and width
//   ens_walk      a workgroup per (flat sequence i, chunk of KA_ENS_JCHUNK sequences j of i's family); col_k[i][.] of every member
//                 is staged in LDS once per workgroup (R x len_i ints, when it fits), each of the four waves takes one j at a
//                 time, its lanes the residues ri.  The res_k[j] rows are read where they lie: a wave reads R rows of 2 * W
//                 bytes for len_i * R lookups, which stay in L1/L2.  SCORE adds into the family's sum with a 64-bit vector
//                 atomic (exact integers: the order does not matter).  COUNT takes every support level n_runs .. minSup of
//                 the family in ONE pass: the n_runs gathers of (i, ri, j) give the level of each distinct partner, and a
//                 wave's per-level counters live in its lanes (lane L - 1 holds level L).  WRITE takes one level at a time.
//                 A launch covers a contiguous range of workgroups from blk0; the counters of a COUNT launch (and the offsets
//                 WRITE reads) are those of its rows only.
//   ens_row_scan  a workgroup per row (level, flat sequence i) of a launch's count table; the [rows][N] block that a table pass
//                 (ka_poar.hip) counts is one level of that layout
//   ens_conf_res  a thread per cell of the X maps, ens_conf_col a thread per flat column: a column's confidences added in row
//                 order in double as the reference adds them
#include <hip/hip_runtime.h>
#include "ka_ens.h"
#include "ka_msa.h"

#define ENS_THREADS 256
#define ENS_WAVES (ENS_THREADS / 64)

// a wave's sum in every lane (ka_msa_wave_sum leaves it in lane 0 alone: COUNT needs it in lane L - 1)
__device__ __forceinline__ int ens_wave_sum_all(int v)
{
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
}

template <int MODE, int RM>
__global__ __launch_bounds__(ENS_THREADS) void ens_walk(KaEnsFamArgs a)
{
        extern __shared__ int lds[];
        const int b = a.blk0 + (int)blockIdx.x;
        const int f = ka_fam_find(a.blkFirst, a.nFam, b);
        const KaEnsFam d = a.fams[f];
        const int t0 = b - a.blkFirst[f];
        const int il = t0 / d.nJC;                               // i and j inside the family
        const int j0 = (t0 % d.nJC) * KA_ENS_JCHUNK;
        const int j1 = min(d.N, j0 + KA_ENS_JCHUNK);
        if (MODE != KA_ENS_CONF && j1 <= il + 1) return;         // only pairs j > i (uniform over the workgroup)
        if (MODE == KA_ENS_WRITE && a.level < d.minSup) return;  // the family stops above this level
        constexpr bool withX = MODE == KA_ENS_SCORE || MODE == KA_ENS_CONF;
        int Wx = 0;
        const int16_t* resX = nullptr;
        if (withX) {
                Wx = a.xW[f];
                if (Wx <= 0) return;                             // a skipped family (uniform)
                resX = a.resX + a.xCell[f];
        }
        const int si = d.firstSeq + il;
        const int li = a.lens[si], oi = a.offs[si], R = a.R;
        int* cxL = lds;                                          // SCORE / CONF: column of X of residue ri
        int* sumL = lds + d.maxlen;                              // CONF: per-residue sums of this workgroup
        int* npL = lds + 2 * d.maxlen;
        int* colL = lds + (withX ? 3 * d.maxlen : 0);            // [R][li] when staged (COUNT / WRITE: nothing else)
        const int* colP;
        long long cs;
        if (d.colInLds) {
                for (int t = threadIdx.x; t < R * li; t += ENS_THREADS) {
                        const int k = t / li;
                        colL[t] = a.col[(long long)k * a.T + oi + (t - k * li)];
                }
                colP = colL; cs = li;
        } else {
                colP = a.col + oi; cs = a.T;
        }
        if (withX)
                for (int t = threadIdx.x; t < li; t += ENS_THREADS) {
                        cxL[t] = a.colX[oi + t];
                        if (MODE == KA_ENS_CONF) { sumL[t] = 0; npL[t] = 0; }
                }
        __syncthreads();
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        long long acc = 0;
        long long famK[RM];                                      // this family in member k's res map, and its width (uniform; read once:
        int wK[RM];                                              // the stores of WRITE would have them read again for every j)
#pragma unroll
        for (int k = 0; k < RM; k++) {
                famK[k] = k < R ? a.resBase[k] + a.memCell[(long long)k * (a.nFam + 1) + f] : 0;
                wK[k] = k < R ? a.memW[(long long)k * a.nFam + f] : 0;
        }
        for (int j = j0 + wave; j < j1; j += ENS_WAVES) {
                if (MODE == KA_ENS_CONF ? j == il : j <= il) continue;
                const int oj = a.offs[d.firstSeq + j];
                long long rowK[RM];                              // row j of the family in member k's res map (wave-uniform)
#pragma unroll
                for (int k = 0; k < RM; k++) rowK[k] = famK[k] + (long long)j * wK[k];
                int perLevel = 0;                                // COUNT: lane L - 1 counts level L
                const long long cell = d.cntFirst + (long long)il * d.N + j - a.cnt0;   // COUNT / WRITE: the pair in a level of the count table
                long long base = 0;                              // WRITE: the pair's next slot
                if (MODE == KA_ENS_WRITE)
                        base = a.rowBase[(long long)(R - a.level) * a.rows + si - a.row0] + a.pairOff[(long long)(R - a.level) * a.E + cell];
                for (int rb = 0; rb < li; rb += 64) {
                        const int ri = rb + lane;
                        const bool ok = ri < li;
                        if (withX) {
                                if (!ok) continue;
                                const int rj = resX[(long long)j * Wx + cxL[ri]];
                                if (rj < 0) continue;
                                int sup = 0;
#pragma unroll
                                for (int k = 0; k < RM; k++)
                                        if (k < R) sup += a.res[rowK[k] + colP[k * cs + ri]] == rj;
                                if (MODE == KA_ENS_SCORE) acc += sup - 1;
                                else { atomicAdd(&sumL[ri], sup); atomicAdd(&npL[ri], 1); }
                        } else {
                                // the residues of j that the members put next to (i, ri); lev[k]: the number of members that hold
                                // v[k], at the first k that holds it (0 elsewhere and at gaps) -- its support level
                                int v[RM], lev[RM];
#pragma unroll
                                for (int k = 0; k < RM; k++)
                                        v[k] = (ok && k < R) ? (int)a.res[rowK[k] + colP[k * cs + ri]] : -1;
#pragma unroll
                                for (int k = 0; k < RM; k++) {
                                        int m = 0;
                                        bool first = true;
#pragma unroll
                                        for (int k2 = 0; k2 < RM; k2++) {
                                                m += v[k2] == v[k];
                                                if (k2 < k && v[k2] == v[k]) first = false;
                                        }
                                        lev[k] = (v[k] >= 0 && first) ? m : 0;
                                }
                                if (MODE == KA_ENS_COUNT) {
                                        for (int L = d.minSup; L <= R; L++) {
                                                int c = 0;
#pragma unroll
                                                for (int k = 0; k < RM; k++) c += lev[k] == L;
                                                c = ens_wave_sum_all(c);
                                                if (lane == L - 1) perLevel += c;
                                        }
                                        continue;
                                }
                                // WRITE, one level: the distinct partners held by exactly `level` members, in ascending order (the
                                // reference's key order ri << 20 | rj)
                                unsigned q = 0;
#pragma unroll
                                for (int k = 0; k < RM; k++) q |= (unsigned)(lev[k] == a.level) << k;
                                const int c = __popc(q);
                                const int incl = ens_wave_incl_scan(c, lane);
                                const int total = __shfl(incl, 63, 64);
                                const long long at = base + incl - c;
#pragma unroll
                                for (int k = 0; k < RM; k++) {
                                        if (!(q >> k & 1u)) continue;
                                        int rank = 0;
#pragma unroll
                                        for (int k2 = 0; k2 < RM; k2++) rank += (q >> k2 & 1u) && v[k2] < v[k];
                                        a.out[at + rank] = make_int2(oi - d.firstRes + ri, oj - d.firstRes + v[k]);
                                }
                                base += total;
                        }
                }
                if (MODE == KA_ENS_COUNT && lane < R && lane + 1 >= d.minSup)
                        a.cnt[(long long)(R - 1 - lane) * a.E + cell] = perLevel;
        }
        if (MODE == KA_ENS_SCORE) {
                const long long t = ka_msa_wave_sum(acc);
                if (lane == 0 && t) atomicAdd(&a.score[f], (unsigned long long)t);
        }
        if (MODE == KA_ENS_CONF) {
                __syncthreads();
                for (int t = threadIdx.x; t < li; t += ENS_THREADS)
                        if (npL[t]) { atomicAdd(&a.supSum[oi + t], sumL[t]); atomicAdd(&a.nPair[oi + t], npL[t]); }
        }
}

// one workgroup per row (level, flat sequence i) of the launch's count table: exclusive scan of the pair counts over j, and the row's total
__global__ __launch_bounds__(ENS_THREADS) void ens_row_scan(KaEnsFamArgs a, long long* pairOff, long long* rowTot)
{
        __shared__ long long wsum[ENS_WAVES];
        const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int lv = r / a.rows, si = a.row0 + r - lv * a.rows;
        const int f = ka_fam_find(a.firstSeq, a.nFam, si);
        const int N = a.fams[f].N;
        const long long at = (long long)lv * a.E + a.fams[f].cntFirst + (long long)(si - a.firstSeq[f]) * N - a.cnt0;
        const int* c = a.cnt + at;
        long long* po = pairOff + at;
        long long run = 0;
        for (int b = 0; b < N; b += ENS_THREADS) {
                const int j = b + threadIdx.x;
                const int v = j < N ? c[j] : 0;
                const int incl = ens_wave_incl_scan(v, lane);
                if (lane == 63) wsum[wave] = incl;
                __syncthreads();
                long long before = run;
                for (int w = 0; w < wave; w++) before += wsum[w];
                if (j < N) po[j] = before + incl - v;
                long long tot = 0;
                for (int w = 0; w < ENS_WAVES; w++) tot += wsum[w];
                __syncthreads();
                run += tot;
        }
        if (threadIdx.x == 0) rowTot[r] = run;
}

// compute_residue_confidence (consensus_msa.c:564-692): per residue (float)(sum / ((double)n_pairs * n_runs)), gaps 0
__global__ void ens_conf_res(KaEnsFamArgs a, float* conf)
{
        const long long tt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (tt >= a.xCell[a.nFam]) return;
        const int t = (int)tt, f = ka_fam_find(a.xCell, a.nFam, t);
        const int s = a.firstSeq[f] + (t - a.xCell[f]) / a.xW[f];
        const int r = a.resX[t];
        float v = 0.0f;
        if (r >= 0) {
                const int e = a.offs[s] + r;
                const int np = a.nPair[e];
                if (np > 0) v = (float)((double)a.supSum[e] / ((double)np * (double)a.R));
        }
        conf[t] = v;
}

// ... per column: the residues' confidences added in row order in double, (float)(sum / count)
__global__ void ens_conf_col(KaEnsFamArgs a, const float* conf, float* colConf)
{
        const long long cc = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (cc >= a.xCol[a.nFam]) return;
        const int c = (int)cc, f = ka_fam_find(a.xCol, a.nFam, c);
        const int W = a.xW[f], N = a.fams[f].N;
        const long long at = (long long)a.xCell[f] + (c - a.xCol[f]);
        double sum = 0.0;
        int count = 0;
        for (int s = 0; s < N; s++)
                if (a.resX[at + (long long)s * W] >= 0) { sum += conf[at + (long long)s * W]; count++; }
        colConf[c] = count > 0 ? (float)(sum / count) : 0.0f;
}

template <int MODE>
static void walk(const KaEnsFamArgs& a, int nBlocks, size_t lds, hipStream_t s)
{
        if (nBlocks <= 0) return;
        if (a.R <= 8) ens_walk<MODE, 8><<<(unsigned)nBlocks, ENS_THREADS, lds, s>>>(a);
        else ens_walk<MODE, KA_ENS_MAX_RUNS><<<(unsigned)nBlocks, ENS_THREADS, lds, s>>>(a);
}

void ka_ens_launch_walk(int mode, const KaEnsFamArgs& a, int nBlocks, size_t lds, hipStream_t s)
{
        switch (mode) {
        case KA_ENS_SCORE: walk<KA_ENS_SCORE>(a, nBlocks, lds, s); break;
        case KA_ENS_CONF: walk<KA_ENS_CONF>(a, nBlocks, lds, s); break;
        case KA_ENS_COUNT: walk<KA_ENS_COUNT>(a, nBlocks, lds, s); break;
        default: walk<KA_ENS_WRITE>(a, nBlocks, lds, s); break;
        }
}

void ka_ens_launch_row_scan(const KaEnsFamArgs& a, int nRows, long long* pairOff, long long* rowTot, hipStream_t s)
{
        if (nRows > 0) ens_row_scan<<<nRows, ENS_THREADS, 0, s>>>(a, pairOff, rowTot);
}

void ka_ens_launch_conf(const KaEnsFamArgs& a, int cells, int cols, float* conf, float* colConf, hipStream_t s)
{
        ens_conf_res<<<(unsigned)(((long long)cells + 255) / 256), 256, 0, s>>>(a, conf);
        ens_conf_col<<<(unsigned)(((long long)cols + 255) / 256), 256, 0, s>>>(a, conf, colConf);
}
