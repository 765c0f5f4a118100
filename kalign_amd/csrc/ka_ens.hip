// ka_ens.hip -- the ensemble consensus stage on the device (kalign_ensemble's tail, lib/src/ensemble.c:341-; poar.c,
// consensus_msa.c).
//
// The reference keeps, for every pair of sequences, a sorted table of the residue pairs (POARs) that some member
// aligns, with a bit per member.  The table is a function of the members' position maps: with col_k[s][r] the column
// of residue r of sequence s in member k and res_k[s][c] the residue of s at column c of member k (or -1),
//     support(i, ri, j, rj) = #{ k : res_k[j][col_k[i][ri]] == rj }  ( = #{ k : col_k[i][ri] == col_k[j][rj] } ).
// So every quantity of the stage is an integer count of n_runs gathers per (i, ri, j):
//   SCORE  sum over the aligned pairs of an alignment X of (support - 1)        (score_alignment_poar, exact int64)
//   CONF   per residue of X: sum of support over its partners, number of partners (compute_residue_confidence)
//   COUNT  per pair (i, j): distinct (ri, rj) with support == level              (build_consensus' candidate list,
//   WRITE  ... and the candidates themselves, in the reference's order           one support level at a time)
// One walk serves all four: a workgroup takes one sequence i and KA_ENS_JCHUNK sequences j; col_k[i][.] of every
// member is staged in LDS once per workgroup (R x len_i ints), each of the four waves takes one j at a time, its lanes
// the residues ri.  The res_k[j] rows are read where they lie: a wave reads R rows of 2 * W bytes for len_i * R
// lookups, which stay in L1/L2.
#include <hip/hip_runtime.h>
#include "ka_ens.h"
#include "ka_msa.h"

#define ENS_THREADS 256

template <int MODE, int RM>
__global__ __launch_bounds__(ENS_THREADS) void ens_walk(KaEnsArgs a)
{
        extern __shared__ int lds[];
        const int nJC = (a.N + KA_ENS_JCHUNK - 1) / KA_ENS_JCHUNK;
        const int i = a.i0 + (int)blockIdx.x / nJC;
        const int j0 = ((int)blockIdx.x % nJC) * KA_ENS_JCHUNK;
        const int j1 = min(a.N, j0 + KA_ENS_JCHUNK);
        if (MODE != KA_ENS_CONF && j1 <= i + 1) return;          // only pairs j > i (uniform over the workgroup)
        const int li = a.lens[i], oi = a.offs[i], R = a.R;
        constexpr bool withX = MODE == KA_ENS_SCORE || MODE == KA_ENS_CONF;
        int* cxL = lds;                                          // SCORE / CONF: column of X of residue ri
        int* sumL = lds + a.maxlen;                              // CONF: per-residue sums of this workgroup
        int* npL = lds + 2 * a.maxlen;
        int* colL = lds + (withX ? 3 * a.maxlen : 0);            // [R][li] when staged (COUNT / WRITE: nothing else)
        const int* colP;
        long long cs;
        if (a.colInLds) {
                for (int t = threadIdx.x; t < R * li; t += ENS_THREADS) {
                        const int k = t / li;
                        colL[t] = a.col[(long long)k * a.T + oi + (t - k * li)];
                }
                colP = colL; cs = li;
        } else {
                colP = a.col + oi; cs = a.T;
        }
        if (MODE == KA_ENS_SCORE || MODE == KA_ENS_CONF)
                for (int t = threadIdx.x; t < li; t += ENS_THREADS) {
                        cxL[t] = a.colX[oi + t];
                        if (MODE == KA_ENS_CONF) { sumL[t] = 0; npL[t] = 0; }
                }
        __syncthreads();
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        long long acc = 0;
        for (int j = j0 + wave; j < j1; j += ENS_THREADS / 64) {
                if (MODE == KA_ENS_CONF ? j == i : j <= i) continue;
                long long base = 0;
                if (MODE == KA_ENS_WRITE) base = a.rowBase[i - a.i0] + a.pairOff[(long long)(i - a.i0) * a.N + j];
                const int oj = a.offs[j];
                int cntj = 0;
                for (int rb = 0; rb < li; rb += 64) {
                        const int ri = rb + lane;
                        const bool ok = ri < li;
                        if (MODE == KA_ENS_SCORE || MODE == KA_ENS_CONF) {
                                if (!ok) continue;
                                const int rj = a.resX[(long long)j * a.Wx + cxL[ri]];
                                if (rj < 0) continue;
                                int sup = 0;
#pragma unroll
                                for (int k = 0; k < RM; k++)
                                        if (k < R) sup += a.res[a.resOff[k] + (long long)j * a.W[k] + colP[k * cs + ri]] == rj;
                                if (MODE == KA_ENS_SCORE) acc += sup - 1;
                                else { atomicAdd(&sumL[ri], sup); atomicAdd(&npL[ri], 1); }
                        } else {
                                // the residues of j that the members put next to (i, ri); the distinct ones held by exactly
                                // `level` members, in ascending order (the reference's key order ri << 20 | rj)
                                int v[RM];
#pragma unroll
                                for (int k = 0; k < RM; k++)
                                        v[k] = (ok && k < R) ? (int)a.res[a.resOff[k] + (long long)j * a.W[k] + colP[k * cs + ri]] : -1;
                                unsigned q = 0;
#pragma unroll
                                for (int k = 0; k < RM; k++) {
                                        int m = 0;
                                        bool first = true;
#pragma unroll
                                        for (int k2 = 0; k2 < RM; k2++) {
                                                m += v[k2] == v[k];
                                                if (k2 < k && v[k2] == v[k]) first = false;
                                        }
                                        if (v[k] >= 0 && first && m == a.level) q |= 1u << k;
                                }
                                const int c = __popc(q);
                                if (MODE == KA_ENS_COUNT) { cntj += c; continue; }
                                const int incl = ens_wave_incl_scan(c, lane);
                                const int total = __shfl(incl, 63, 64);
                                long long at = base + incl - c;
#pragma unroll
                                for (int k = 0; k < RM; k++) {
                                        if (!(q >> k & 1u)) continue;
                                        int rank = 0;
#pragma unroll
                                        for (int k2 = 0; k2 < RM; k2++) rank += (q >> k2 & 1u) && v[k2] < v[k];
                                        a.out[at + rank] = make_int2(oi + ri, oj + v[k]);
                                }
                                base += total;
                        }
                }
                if (MODE == KA_ENS_COUNT) {
                        const long long t = ka_msa_wave_sum(cntj);
                        if (lane == 0) a.cnt[(long long)(i - a.i0) * a.N + j] = (int)t;
                }
        }
        if (MODE == KA_ENS_SCORE) {
                const long long t = ka_msa_wave_sum(acc);
                if (lane == 0 && t) atomicAdd(a.score, (unsigned long long)t);
        }
        if (MODE == KA_ENS_CONF) {
                __syncthreads();
                for (int t = threadIdx.x; t < li; t += ENS_THREADS)
                        if (npL[t]) { atomicAdd(&a.supSum[oi + t], sumL[t]); atomicAdd(&a.nPair[oi + t], npL[t]); }
        }
}

// one workgroup per row i of the chunk: exclusive scan of the pair counts over j, and the row's total
__global__ __launch_bounds__(ENS_THREADS) void ens_row_scan(const int* cnt, int N, long long* pairOff, long long* rowTot)
{
        __shared__ long long wsum[ENS_THREADS / 64];
        const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int* c = cnt + (long long)i * N;
        long long* po = pairOff + (long long)i * N;
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
                for (int w = 0; w < ENS_THREADS / 64; w++) tot += wsum[w];
                __syncthreads();
                run += tot;
        }
        if (threadIdx.x == 0) rowTot[i] = run;
}

// compute_residue_confidence (consensus_msa.c:564-692): per residue (float)(sum / ((double)n_pairs * n_runs)), gaps 0
__global__ void ens_conf_res(KaEnsArgs a, float* conf)
{
        const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (t >= (long long)a.N * a.Wx) return;
        const int s = (int)(t / a.Wx);
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
__global__ void ens_conf_col(KaEnsArgs a, const float* conf, float* colConf)
{
        const int c = blockIdx.x * blockDim.x + threadIdx.x;
        if (c >= a.Wx) return;
        double sum = 0.0;
        int count = 0;
        for (int s = 0; s < a.N; s++)
                if (a.resX[(long long)s * a.Wx + c] >= 0) { sum += conf[(long long)s * a.Wx + c]; count++; }
        colConf[c] = count > 0 ? (float)(sum / count) : 0.0f;
}

template <int MODE>
static void walk(const KaEnsArgs& a, hipStream_t s)
{
        const int nJC = (a.N + KA_ENS_JCHUNK - 1) / KA_ENS_JCHUNK;
        const long long blocks = (long long)(a.i1 - a.i0) * nJC;
        if (blocks <= 0) return;
        const bool withX = MODE == KA_ENS_SCORE || MODE == KA_ENS_CONF;
        const size_t lds = (size_t)((withX ? 3 * a.maxlen : 0) + (a.colInLds ? a.R * a.maxlen : 0)) * sizeof(int);
        if (a.R <= 8) ens_walk<MODE, 8><<<(unsigned)blocks, ENS_THREADS, lds, s>>>(a);
        else ens_walk<MODE, KA_ENS_MAX_RUNS><<<(unsigned)blocks, ENS_THREADS, lds, s>>>(a);
}

void ka_ens_launch_walk(int mode, const KaEnsArgs& a, hipStream_t s)
{
        switch (mode) {
        case KA_ENS_SCORE: walk<KA_ENS_SCORE>(a, s); break;
        case KA_ENS_CONF: walk<KA_ENS_CONF>(a, s); break;
        case KA_ENS_COUNT: walk<KA_ENS_COUNT>(a, s); break;
        default: walk<KA_ENS_WRITE>(a, s); break;
        }
}

void ka_ens_launch_row_scan(const int* cnt, int N, long long* pairOff, long long* rowTot, int rows, hipStream_t s)
{
        ens_row_scan<<<rows, ENS_THREADS, 0, s>>>(cnt, N, pairOff, rowTot);
}

void ka_ens_launch_conf(const KaEnsArgs& a, float* conf, float* colConf, hipStream_t s)
{
        const long long n = (long long)a.N * a.Wx;
        ens_conf_res<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(a, conf);
        ens_conf_col<<<(a.Wx + 255) / 256, 256, 0, s>>>(a, conf, colConf);
}
