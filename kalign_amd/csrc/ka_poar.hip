// ka_poar.hip -- the ensemble's table of pairs of aligned residues (POAR; lib/src/poar.c) on the device: built from the
// members when a caller wants the file (poar_table_write, poar.c:203-252), and as the source of support of a handle that
// was opened from such a file (poar_table_read, kalign_consensus_from_poar; poar.c:254-325, ensemble.c:500-543).
//
// Per pair i < j the table holds the distinct (ri, rj) some member aligns, key = ri << 20 | rj ascending, each with a mask
// of the members that hold it.  Every kernel here has the geometry of ens_walk (ka_ens.hip): a workgroup takes one
// sequence i and KA_ENS_JCHUNK sequences j, each of its four waves one j at a time.
//   poar_table   from the members' maps: lanes are the residues ri; a lane's distinct partners rj = res_k[j][col_k[i][ri]]
//                ranked by rj, the mask the OR over the members that gave it (ens_walk's candidates without the level filter)
//   poar_level   from a loaded table: the entries of pair (i, j) whose popcount is the level, compacted in table order into
//                the candidates (element of i, element of j) the greedy takes; level 0: every entry as it is
//   poar_lookup  SCORE / CONF of an alignment X with support = popcount of the entry (ri, rj), found by bisection
#include <hip/hip_runtime.h>
#include "ka_ens.h"
#include "ka_msa.h"

#define POAR_THREADS 256

template <int MODE, int RM>
__global__ __launch_bounds__(POAR_THREADS) void poar_table(KaEnsArgs a)
{
        extern __shared__ int lds[];
        const int nJC = (a.N + KA_ENS_JCHUNK - 1) / KA_ENS_JCHUNK;
        const int i = a.i0 + (int)blockIdx.x / nJC;
        const int j0 = ((int)blockIdx.x % nJC) * KA_ENS_JCHUNK;
        const int j1 = min(a.N, j0 + KA_ENS_JCHUNK);
        if (j1 <= i + 1) return;                                 // only pairs j > i (uniform over the workgroup)
        const int li = a.lens[i], oi = a.offs[i], R = a.R;
        const int* colP;
        long long cs;
        if (a.colInLds) {
                for (int t = threadIdx.x; t < R * li; t += POAR_THREADS) {
                        const int k = t / li;
                        lds[t] = a.col[(long long)k * a.T + oi + (t - k * li)];
                }
                colP = lds; cs = li;
        } else {
                colP = a.col + oi; cs = a.T;
        }
        __syncthreads();
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int j = max(j0, i + 1) + wave; j < j1; j += POAR_THREADS / 64) {
                long long base = 0;
                if (MODE == KA_ENS_WRITE) base = a.rowBase[i - a.i0] + a.pairOff[(long long)(i - a.i0) * a.N + j];
                int cntj = 0;
                for (int rb = 0; rb < li; rb += 64) {
                        const int ri = rb + lane;
                        const bool ok = ri < li;
                        int v[RM];
#pragma unroll
                        for (int k = 0; k < RM; k++)
                                v[k] = (ok && k < R) ? (int)a.res[a.resOff[k] + (long long)j * a.W[k] + colP[k * cs + ri]] : -1;
                        // bit k of q: member k is the first to name its partner
                        unsigned q = 0;
#pragma unroll
                        for (int k = 0; k < RM; k++) {
                                bool first = v[k] >= 0;
#pragma unroll
                                for (int k2 = 0; k2 < k; k2++)
                                        if (v[k2] == v[k]) first = false;
                                if (first) q |= 1u << k;
                        }
                        const int c = __popc(q);
                        if (MODE == KA_ENS_COUNT) { cntj += c; continue; }
                        const int incl = ens_wave_incl_scan(c, lane);
                        const int total = __shfl(incl, 63, 64);
                        const long long at = base + incl - c;
#pragma unroll
                        for (int k = 0; k < RM; k++) {
                                if (!(q >> k & 1u)) continue;
                                int rank = 0;
                                unsigned mask = 0;
#pragma unroll
                                for (int k2 = 0; k2 < RM; k2++) {
                                        rank += (q >> k2 & 1u) && v[k2] < v[k];
                                        if (v[k2] == v[k]) mask |= 1u << k2;
                                }
                                a.entOut[at + rank] = make_uint2((unsigned)ri << 20 | (unsigned)v[k], mask);
                        }
                        base += total;
                }
                if (MODE == KA_ENS_COUNT) {
                        const long long t = ka_msa_wave_sum(cntj);
                        if (lane == 0) a.cnt[(long long)(i - a.i0) * a.N + j] = (int)t;
                }
        }
}

template <int MODE>
__global__ __launch_bounds__(POAR_THREADS) void poar_level(KaEnsArgs a)
{
        const int nJC = (a.N + KA_ENS_JCHUNK - 1) / KA_ENS_JCHUNK;
        const int i = a.i0 + (int)blockIdx.x / nJC;
        const int j0 = ((int)blockIdx.x % nJC) * KA_ENS_JCHUNK;
        const int j1 = min(a.N, j0 + KA_ENS_JCHUNK);
        if (j1 <= i + 1) return;
        const int oi = a.offs[i];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int j = max(j0, i + 1) + wave; j < j1; j += POAR_THREADS / 64) {
                const long long p = ka_poar_pair(i, j, a.N);
                const long long e0 = a.pairStart[p], e1 = a.pairStart[p + 1];
                if (MODE == KA_ENS_COUNT && a.level == 0) {
                        if (lane == 0) a.cnt[(long long)(i - a.i0) * a.N + j] = (int)(e1 - e0);
                        continue;
                }
                long long base = 0;
                if (MODE == KA_ENS_WRITE) base = a.rowBase[i - a.i0] + a.pairOff[(long long)(i - a.i0) * a.N + j];
                const int oj = a.offs[j];
                int cntj = 0;
                for (long long b = e0; b < e1; b += 64) {
                        const long long x = b + lane;
                        uint2 e = make_uint2(0u, 0u);
                        if (x < e1) e = a.ent[x];
                        const bool hit = x < e1 && (a.level == 0 || __popc(e.y) == a.level);
                        if (MODE == KA_ENS_COUNT) { cntj += hit; continue; }
                        const unsigned long long bal = __ballot(hit);
                        if (hit) {
                                const long long at = base + __popcll(bal & ((1ull << lane) - 1ull));
                                if (a.level == 0) a.entOut[at] = e;
                                else a.out[at] = make_int2(oi + (int)(e.x >> 20), oj + (int)(e.x & 0xFFFFFu));
                        }
                        base += __popcll(bal);
                }
                if (MODE == KA_ENS_COUNT) {
                        const long long t = ka_msa_wave_sum(cntj);
                        if (lane == 0) a.cnt[(long long)(i - a.i0) * a.N + j] = (int)t;
                }
        }
}

template <int MODE>
__global__ __launch_bounds__(POAR_THREADS) void poar_lookup(KaEnsArgs a)
{
        extern __shared__ int lds[];
        const int nJC = (a.N + KA_ENS_JCHUNK - 1) / KA_ENS_JCHUNK;
        const int i = a.i0 + (int)blockIdx.x / nJC;
        const int j0 = ((int)blockIdx.x % nJC) * KA_ENS_JCHUNK;
        const int j1 = min(a.N, j0 + KA_ENS_JCHUNK);
        if (MODE != KA_ENS_CONF && j1 <= i + 1) return;
        const int li = a.lens[i], oi = a.offs[i];
        int* cxL = lds;                                          // column of X of residue ri
        int* sumL = lds + a.maxlen;                              // CONF: per-residue sums of this workgroup
        int* npL = lds + 2 * a.maxlen;
        for (int t = threadIdx.x; t < li; t += POAR_THREADS) {
                cxL[t] = a.colX[oi + t];
                if (MODE == KA_ENS_CONF) { sumL[t] = 0; npL[t] = 0; }
        }
        __syncthreads();
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        long long acc = 0;
        for (int j = j0 + wave; j < j1; j += POAR_THREADS / 64) {
                if (MODE == KA_ENS_CONF ? j == i : j <= i) continue;
                // the pair is stored under (min, max); for i > j the key is rj << 20 | ri (consensus_msa.c:624-631)
                const long long p = i < j ? ka_poar_pair(i, j, a.N) : ka_poar_pair(j, i, a.N);
                const long long e0 = a.pairStart[p], e1 = a.pairStart[p + 1];
                for (int ri = lane; ri < li; ri += 64) {
                        const int rj = a.resX[(long long)j * a.Wx + cxL[ri]];
                        if (rj < 0) continue;
                        const unsigned key = i < j ? (unsigned)ri << 20 | (unsigned)rj : (unsigned)rj << 20 | (unsigned)ri;
                        long long lo = e0, hi = e1;                  // first entry with key >= ours
                        while (lo < hi) {
                                const long long mid = (lo + hi) >> 1;
                                if (a.ent[mid].x < key) lo = mid + 1;
                                else hi = mid;
                        }
                        int sup = 0;
                        if (lo < e1) {
                                const uint2 e = a.ent[lo];
                                if (e.x == key) sup = __popc(e.y);
                        }
                        if (MODE == KA_ENS_SCORE) acc += sup - 1;
                        else { atomicAdd(&sumL[ri], sup); atomicAdd(&npL[ri], 1); }
                }
        }
        if (MODE == KA_ENS_SCORE) {
                const long long t = ka_msa_wave_sum(acc);
                if (lane == 0 && t) atomicAdd(a.score, (unsigned long long)t);
        }
        if (MODE == KA_ENS_CONF) {
                __syncthreads();
                for (int t = threadIdx.x; t < li; t += POAR_THREADS)
                        if (npL[t]) { atomicAdd(&a.supSum[oi + t], sumL[t]); atomicAdd(&a.nPair[oi + t], npL[t]); }
        }
}

static unsigned poar_blocks(const KaEnsArgs& a)
{
        const int nJC = (a.N + KA_ENS_JCHUNK - 1) / KA_ENS_JCHUNK;
        const long long blocks = (long long)(a.i1 - a.i0) * nJC;
        return blocks > 0 ? (unsigned)blocks : 0u;
}

void ka_poar_launch_table(int mode, const KaEnsArgs& a, hipStream_t s)
{
        const unsigned blocks = poar_blocks(a);
        if (!blocks) return;
        const size_t lds = (size_t)(a.colInLds ? a.R * a.maxlen : 0) * sizeof(int);
        if (a.R <= 8) {
                if (mode == KA_ENS_COUNT) poar_table<KA_ENS_COUNT, 8><<<blocks, POAR_THREADS, lds, s>>>(a);
                else poar_table<KA_ENS_WRITE, 8><<<blocks, POAR_THREADS, lds, s>>>(a);
        } else {
                if (mode == KA_ENS_COUNT) poar_table<KA_ENS_COUNT, KA_ENS_MAX_RUNS><<<blocks, POAR_THREADS, lds, s>>>(a);
                else poar_table<KA_ENS_WRITE, KA_ENS_MAX_RUNS><<<blocks, POAR_THREADS, lds, s>>>(a);
        }
}

void ka_poar_launch_level(int mode, const KaEnsArgs& a, hipStream_t s)
{
        const unsigned blocks = poar_blocks(a);
        if (!blocks) return;
        if (mode == KA_ENS_COUNT) poar_level<KA_ENS_COUNT><<<blocks, POAR_THREADS, 0, s>>>(a);
        else poar_level<KA_ENS_WRITE><<<blocks, POAR_THREADS, 0, s>>>(a);
}

void ka_poar_launch_lookup(int mode, const KaEnsArgs& a, hipStream_t s)
{
        const unsigned blocks = poar_blocks(a);
        if (!blocks) return;
        const size_t lds = (size_t)3 * a.maxlen * sizeof(int);
        if (mode == KA_ENS_SCORE) poar_lookup<KA_ENS_SCORE><<<blocks, POAR_THREADS, lds, s>>>(a);
        else poar_lookup<KA_ENS_CONF><<<blocks, POAR_THREADS, lds, s>>>(a);
}
