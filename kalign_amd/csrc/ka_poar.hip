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
//   poar_merge   two tables into one (ka_ens_merge): per pair the sorted union of the keys, the second table's member bits
//                above the first's
//   poar_select  a table with some of its member bits, in a new order (ka_ens_select); an entry that keeps none is dropped
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

// first index in [lo, hi) whose key is >= key (hi when there is none)
__device__ __forceinline__ long long poar_lower_bound(const uint2* ent, long long lo, long long hi, unsigned key)
{
        while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (ent[mid].x < key) lo = mid + 1;
                else hi = mid;
        }
        return lo;
}

// The union of the tables A (a.pairStart / a.ent, a.shift members) and B (a.pairStartB / a.entB) of one set of sequences, B's
// member bits above A's.  A wave takes a pair; its lanes take A's entries in tiles of 64, then B's.  An entry's slot in the
// sorted union is its own index plus the other list's entries below its key (a bisection) minus the keys below it that both
// lists hold -- a ballot prefix inside the tile and a carry across tiles.  A shared key is written by the A side alone, with
// both masks; the B side skips it.  COUNT needs the A side only: |A| + |B| - |A and B|.
template <int MODE>
__global__ __launch_bounds__(POAR_THREADS) void poar_merge(KaEnsArgs a)
{
        const int nJC = (a.N + KA_ENS_JCHUNK - 1) / KA_ENS_JCHUNK;
        const int i = a.i0 + (int)blockIdx.x / nJC;
        const int j0 = ((int)blockIdx.x % nJC) * KA_ENS_JCHUNK;
        const int j1 = min(a.N, j0 + KA_ENS_JCHUNK);
        if (j1 <= i + 1) return;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int j = max(j0, i + 1) + wave; j < j1; j += POAR_THREADS / 64) {
                const long long p = ka_poar_pair(i, j, a.N);
                const long long a0 = a.pairStart[p], a1 = a.pairStart[p + 1];
                const long long b0 = a.pairStartB[p], b1 = a.pairStartB[p + 1];
                const long long base = MODE == KA_ENS_WRITE ? a.outStart[p] : 0;
                long long shared = 0;                                // keys of both lists in the tiles before this one
                for (long long t = a0; t < a1; t += 64) {
                        const long long x = t + lane;
                        uint2 e = make_uint2(0u, 0u);
                        long long lb = b0;
                        unsigned mb = 0;
                        if (x < a1) {
                                e = a.ent[x];
                                lb = poar_lower_bound(a.entB, b0, b1, e.x);
                                if (lb < b1) {
                                        const uint2 f = a.entB[lb];
                                        if (f.x == e.x) mb = f.y;            // (a stored mask is never 0)
                                }
                        }
                        const unsigned long long bal = __ballot(mb != 0);
                        if (MODE == KA_ENS_WRITE && x < a1)
                                a.entOut[base + (x - a0) + (lb - b0) - shared - __popcll(bal & below)] = make_uint2(e.x, e.y | mb << a.shift);
                        shared += __popcll(bal);
                }
                if (MODE == KA_ENS_COUNT) {
                        if (lane == 0) a.cnt[(long long)(i - a.i0) * a.N + j] = (int)((a1 - a0) + (b1 - b0) - shared);
                        continue;
                }
                shared = 0;
                for (long long t = b0; t < b1; t += 64) {
                        const long long y = t + lane;
                        uint2 e = make_uint2(0u, 0u);
                        long long la = a0;
                        bool both = false;
                        if (y < b1) {
                                e = a.entB[y];
                                la = poar_lower_bound(a.ent, a0, a1, e.x);
                                both = la < a1 && a.ent[la].x == e.x;
                        }
                        const unsigned long long bal = __ballot(both);
                        if (y < b1 && !both)
                                a.entOut[base + (y - b0) + (la - a0) - shared - __popcll(bal & below)] = make_uint2(e.x, e.y << a.shift);
                        shared += __popcll(bal);
                }
        }
}

// A table's entries with the member bits a.sel[0 .. nSel) as bits 0 .. nSel - 1, the entries that keep none of them dropped:
// poar_level's ballot compaction with this predicate, table to table.
template <int MODE>
__global__ __launch_bounds__(POAR_THREADS) void poar_select(KaEnsArgs a)
{
        const int nJC = (a.N + KA_ENS_JCHUNK - 1) / KA_ENS_JCHUNK;
        const int i = a.i0 + (int)blockIdx.x / nJC;
        const int j0 = ((int)blockIdx.x % nJC) * KA_ENS_JCHUNK;
        const int j1 = min(a.N, j0 + KA_ENS_JCHUNK);
        if (j1 <= i + 1) return;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int j = max(j0, i + 1) + wave; j < j1; j += POAR_THREADS / 64) {
                const long long p = ka_poar_pair(i, j, a.N);
                const long long e0 = a.pairStart[p], e1 = a.pairStart[p + 1];
                long long base = MODE == KA_ENS_WRITE ? a.outStart[p] : 0;
                int cntj = 0;
                for (long long b = e0; b < e1; b += 64) {
                        const long long x = b + lane;
                        uint2 e = make_uint2(0u, 0u);
                        if (x < e1) e = a.ent[x];
                        unsigned m = 0;
                        for (int t = 0; t < a.nSel; t++) m |= (e.y >> a.sel[t] & 1u) << t;
                        if (MODE == KA_ENS_COUNT) { cntj += m != 0; continue; }
                        const unsigned long long bal = __ballot(m != 0);
                        if (m) a.entOut[base + __popcll(bal & ((1ull << lane) - 1ull))] = make_uint2(e.x, m);
                        base += __popcll(bal);
                }
                if (MODE == KA_ENS_COUNT) {
                        const long long t = ka_msa_wave_sum(cntj);
                        if (lane == 0) a.cnt[(long long)(i - a.i0) * a.N + j] = (int)t;
                }
        }
}

// a counted block of rows in the table's own layout: the first entry of every pair (i, j), i0 <= i < i1
__global__ __launch_bounds__(POAR_THREADS) void poar_pair_start(const long long* pairOff, const long long* rowBase, int i0, int N, long long* pairStart)
{
        const int i = i0 + (int)blockIdx.x;
        for (int j = i + 1 + (int)threadIdx.x; j < N; j += POAR_THREADS)
                pairStart[ka_poar_pair(i, j, N)] = rowBase[i - i0] + pairOff[(long long)(i - i0) * N + j];
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

void ka_poar_launch_merge(int mode, const KaEnsArgs& a, hipStream_t s)
{
        const unsigned blocks = poar_blocks(a);
        if (!blocks) return;
        if (mode == KA_ENS_COUNT) poar_merge<KA_ENS_COUNT><<<blocks, POAR_THREADS, 0, s>>>(a);
        else poar_merge<KA_ENS_WRITE><<<blocks, POAR_THREADS, 0, s>>>(a);
}

void ka_poar_launch_select(int mode, const KaEnsArgs& a, hipStream_t s)
{
        const unsigned blocks = poar_blocks(a);
        if (!blocks) return;
        if (mode == KA_ENS_COUNT) poar_select<KA_ENS_COUNT><<<blocks, POAR_THREADS, 0, s>>>(a);
        else poar_select<KA_ENS_WRITE><<<blocks, POAR_THREADS, 0, s>>>(a);
}

void ka_poar_launch_pair_start(const long long* pairOff, const long long* rowBase, int i0, int i1, int N, long long* pairStart, hipStream_t s)
{
        if (i1 > i0) poar_pair_start<<<i1 - i0, POAR_THREADS, 0, s>>>(pairOff, rowBase, i0, N, pairStart);
}

void ka_poar_launch_lookup(int mode, const KaEnsArgs& a, hipStream_t s)
{
        const unsigned blocks = poar_blocks(a);
        if (!blocks) return;
        const size_t lds = (size_t)3 * a.maxlen * sizeof(int);
        if (mode == KA_ENS_SCORE) poar_lookup<KA_ENS_SCORE><<<blocks, POAR_THREADS, lds, s>>>(a);
        else poar_lookup<KA_ENS_CONF><<<blocks, POAR_THREADS, lds, s>>>(a);
}
