// ka_in.hip -- the kernels of the input stage (gfx950, wave64): raw text of a batch of families -> counts, checksums and
// histograms, then the three encodings in sorted order.  Both walk a sequence's raw bytes a wave per sequence (ka_walk.h).
//   in_scan     a wave per sequence in input order, sixteen consecutive sequences per workgroup.  Residues, gap characters,
//               dropped bytes, the offset of the first byte >= 128 and the GCG checksum per sequence; the family's 128-bin
//               histogram.  A residue's index is the residues before this step, plus the population counts of the step's
//               earlier ballots, plus that of the lower lanes of its own; the lanes' terms (index % 57 + 1) * upper-case byte
//               are summed in 64-bit integers and reduced % 10000 once (the remainder of the sum is what the reference's
//               running remainder comes to; fewer than 2^31 terms below 2^13 each).  The histogram: every wave counts into its own 128 LDS counters by integer
//               atomics; after the barrier one thread per bin folds them into the families' (ka_fold_families).
//   in_encode   a wave per sorted position, four per workgroup.  The same walk; a residue's place is its index, and the wave
//               writes the letter as given, its tree code and its alignment code -- through the two tables of its family's
//               biotype, staged in LDS -- at the position's 64-bit offset in the three planes.  A letter without a code is
//               written as code 0 and counted per family.  A write is held inside the position's own range regardless.
#include "ka_in.h"
#include "ka_msa.h"          // ka_fam_find
#include "ka_walk.h"

namespace {

__global__ __launch_bounds__(KA_IN_SCAN_THREADS) void in_scan(KaInTab a)
{
        constexpr int kWaves = KA_IN_SCAN_THREADS / 64;
        __shared__ unsigned hist[kWaves][KA_IN_BINS];            // (a sequence holds fewer than 2^31 bytes)
        __shared__ int famOf[kWaves];                            // -1: no sequence
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const long long i = (long long)blockIdx.x * kWaves + wave;
        for (int k = lane; k < KA_IN_BINS; k += 64) hist[wave][k] = 0;   // (its own wave's: read by others after the barrier only)
        int f = -1;
        if (i < a.nSeq) {                                        // (the whole wave)
                f = ka_fam_find(a.famFirst, a.nFam, (int)i);
                const uint8_t* raw = a.text + a.seqOff[i];
                const long long n = a.seqOff[i + 1] - a.seqOff[i];
                const unsigned long long below = ka_lanes_below(lane);
                long long residues = 0, gaps = 0, dropped = 0, bad = -1, chk = 0;
                for (long long c0 = 0; c0 < n; c0 += KA_IN_STEP) {
                        int b[KA_IN_STEP / 64];
                        ka_walk_step<KA_IN_STEP>(raw, n, c0, lane, b);
#pragma unroll
                        for (int q = 0; q < KA_IN_STEP / 64; q++) {
                                const bool res = ka_in_is_letter(b[q]), pun = ka_in_is_punct(b[q]);
                                const unsigned long long mr = __ballot(res), mp = __ballot(pun), mh = __ballot(b[q] >= 128),
                                                         ma = __ballot(b[q] >= 0);
                                if (mh && bad < 0) bad = c0 + 64 * q + __ffsll((long long)mh) - 1;
                                if (res) {
                                        const long long j = residues + __popcll(mr & below);
                                        chk += (j % 57 + 1) * (long long)(b[q] & ~32);   // (a letter: clearing bit 5 is toupper)
                                }
                                if (b[q] >= 0 && b[q] < 128) atomicAdd(&hist[wave][b[q]], 1u);
                                residues += __popcll(mr);
                                gaps += __popcll(mp);
                                dropped += __popcll(ma & ~(mr | mp | mh));
                        }
                }
                chk = ka_wave_sum(chk) % 10000;
                const long long rec = lane == KA_IN_RESIDUES ? residues : lane == KA_IN_GAPS ? gaps : lane == KA_IN_DROPPED ? dropped :
                                      lane == KA_IN_CHECKSUM ? chk : bad;
                if (lane < KA_IN_DEVREC) a.recs[i * KA_IN_DEVREC + lane] = (int)rec;
        }
        if (lane == 0) famOf[wave] = f;
        __syncthreads();
        if (threadIdx.x < KA_IN_BINS) ka_fold_families(hist, famOf, threadIdx.x, a.freq, KA_IN_BINS);
}

__global__ __launch_bounds__(KA_IN_ENC_THREADS) void in_encode(KaInTab a)
{
        __shared__ int8_t tab[KA_IN_TABLES * 128];
        for (int k = threadIdx.x; k < KA_IN_TABLES * 128; k += KA_IN_ENC_THREADS) tab[k] = a.tables[k];
        __syncthreads();
        const int lane = threadIdx.x & 63;
        const long long p = (long long)blockIdx.x * (KA_IN_ENC_THREADS / 64) + (threadIdx.x >> 6);
        if (p >= a.nSeq) return;
        const long long n = a.outOff[p + 1] - a.outOff[p];
        if (n <= 0) return;
        const int i = a.order[p];
        const int f = ka_fam_find(a.famFirst, a.nFam, (int)p);
        const bool dna = a.biotype[f] != 0;
        const int8_t* tTree = tab + (dna ? 0 : 128);
        const int8_t* tAln = tab + (dna ? 0 : 256);
        const uint8_t* raw = a.text + a.seqOff[i];
        const long long len = a.seqOff[i + 1] - a.seqOff[i];
        const unsigned long long below = ka_lanes_below(lane);
        const long long o = a.outOff[p];
        long long run = 0, missing = 0;
        for (long long c0 = 0; c0 < len && run < n; c0 += KA_IN_STEP) {
                int b[KA_IN_STEP / 64];
                ka_walk_step<KA_IN_STEP>(raw, len, c0, lane, b);
#pragma unroll
                for (int q = 0; q < KA_IN_STEP / 64; q++) {
                        const bool res = ka_in_is_letter(b[q]);
                        const unsigned long long mr = __ballot(res);
                        const long long j = run + __popcll(mr & below);
                        bool none = false;
                        if (res && j < n) {
                                const int t = tTree[b[q]], c = tAln[b[q]];
                                none = c < 0;
                                a.letters[o + j] = (uint8_t)b[q];
                                a.treeCodes[o + j] = (uint8_t)(t < 0 ? 0 : t);
                                a.codes[o + j] = (uint8_t)(c < 0 ? 0 : c);
                        }
                        missing += __popcll(__ballot(none));
                        run += __popcll(mr);
                }
        }
        if (lane == 0 && missing) atomicAdd(&a.noCode[f], (unsigned long long)missing);
}

} // namespace

void ka_in_run_scan(const KaInTab& a, hipStream_t s, int* launches)
{
        in_scan<<<ka_wave_grid(a.nSeq, KA_IN_SCAN_THREADS), KA_IN_SCAN_THREADS, 0, s>>>(a);
        ++*launches;
}

void ka_in_run_encode(const KaInTab& a, hipStream_t s, int* launches)
{
        in_encode<<<ka_wave_grid(a.nSeq, KA_IN_ENC_THREADS), KA_IN_ENC_THREADS, 0, s>>>(a);
        ++*launches;
}
