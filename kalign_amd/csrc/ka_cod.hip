// ka_cod.hip -- the kernels of the codon stage (gfx950, wave64): raw coding DNA of a batch of families -> upper-cased
// residues, proteins and stop-free codons, and protein rows -> codon rows.  A wave per sequence or row, four per workgroup;
// the walks are ka_walk.h's.
//   cod_pack       a sequence's raw bytes: residues, gap characters, dropped bytes and the offset of the first byte >= 128;
//                  the residues, upper-cased, compacted from seqOff[i] on in a plane the size of the text.
//   cod_translate  a codon per lane, 64 a step: three packed residues -> 2-bit codes -> the 64-letter table staged in LDS, X
//                  for a codon with a letter outside A C G T.  The ballot of the codons that are no stop places the amino
//                  acid in the protein plane and the codon's three bytes in the stop-free codon plane, both from seqOff[i]
//                  on.  Codons, stops and X codons join the record.  It reads the residue count cod_pack left in the
//                  record: the two launches stand back to back in one stream.
//   cod_back       a protein row of W columns: a gap byte becomes three gap bytes at columns 3j .. 3j + 2, the k-th
//                  non-gap byte the k-th kept codon of the row's sequence (three gap bytes past the sequence's last: the
//                  host refuses such a row from the count before any row is handed out); a 0 byte ends the row.  The
//                  row's non-gap count goes to count[row].
// Every store is held inside the sequence's or row's own range regardless of what the bytes say.
#include "ka_cod.h"
#include "ka_msa.h"          // ka_fam_find
#include "ka_walk.h"

namespace {

__global__ __launch_bounds__(KA_COD_THREADS) void cod_pack(KaCodTab a)
{
        const int lane = threadIdx.x & 63;
        const long long i = (long long)blockIdx.x * (KA_COD_THREADS / 64) + (threadIdx.x >> 6);
        if (i >= a.nSeq) return;                                 // (the whole wave)
        const long long o = a.seqOff[i], n = a.seqOff[i + 1] - o;
        const uint8_t* raw = a.text + o;
        uint8_t* out = a.packed + o;
        const unsigned long long below = ka_lanes_below(lane);
        long long residues = 0, gaps = 0, dropped = 0, bad = -1;
        for (long long c0 = 0; c0 < n; c0 += KA_IN_STEP) {
                int b[KA_IN_STEP / 64];
                ka_walk_step<KA_IN_STEP>(raw, n, c0, lane, b);
#pragma unroll
                for (int q = 0; q < KA_IN_STEP / 64; q++) {
                        const bool res = ka_in_is_letter(b[q]), pun = ka_in_is_punct(b[q]);
                        const unsigned long long mr = __ballot(res), mp = __ballot(pun), mh = __ballot(b[q] >= 128), ma = __ballot(b[q] >= 0);
                        if (mh && bad < 0) bad = c0 + 64 * q + __ffsll((long long)mh) - 1;
                        const long long j = residues + __popcll(mr & below);
                        if (res && j < n) out[j] = (uint8_t)(b[q] & ~32);        // (a letter: clearing bit 5 is toupper)
                        residues += __popcll(mr);
                        gaps += __popcll(mp);
                        dropped += __popcll(ma & ~(mr | mp | mh));
                }
        }
        const long long rec = lane == KA_COD_RESIDUES ? residues : lane == KA_COD_GAPS ? gaps : lane == KA_COD_DROPPED ? dropped : bad;
        if (lane <= KA_COD_DROPPED || lane == KA_COD_BAD) a.recs[i * KA_COD_DEVREC + lane] = (int)rec;
}

__global__ __launch_bounds__(KA_COD_THREADS) void cod_translate(KaCodTab a)
{
        __shared__ uint8_t tab[64];
        if (threadIdx.x < 64) tab[threadIdx.x] = a.table[threadIdx.x];
        __syncthreads();
        const int lane = threadIdx.x & 63;
        const long long i = (long long)blockIdx.x * (KA_COD_THREADS / 64) + (threadIdx.x >> 6);
        if (i >= a.nSeq) return;                                 // (the whole wave)
        const long long o = a.seqOff[i], n = a.seqOff[i + 1] - o;
        // (a residue count that is no multiple of 3 is the host's to refuse: the codons it holds in full are translated)
        const long long nCod = min((long long)a.recs[i * KA_COD_DEVREC + KA_COD_RESIDUES], n) / 3;
        const uint8_t* in = a.packed + o;
        uint8_t* prot = a.protein + o;
        uint8_t* kept = a.kept + o;
        const unsigned long long below = ka_lanes_below(lane);
        long long run = 0, stops = 0, xs = 0;
        for (long long c0 = 0; c0 < nCod; c0 += 64) {
                const long long c = c0 + lane;
                const bool valid = c < nCod;
                int r0 = 0, r1 = 0, r2 = 0, aa = 0;
                bool x = false;
                if (valid) {
                        r0 = in[3 * c]; r1 = in[3 * c + 1]; r2 = in[3 * c + 2];
                        const int k0 = ka_cod_code(r0), k1 = ka_cod_code(r1), k2 = ka_cod_code(r2);
                        x = (k0 | k1 | k2) < 0;
                        aa = x ? 'X' : tab[(16 * k0 + 4 * k1 + k2) & 63];
                }
                const bool stop = valid && aa == '*', keep = valid && !stop;
                const unsigned long long mk = __ballot(keep);
                const long long j = run + __popcll(mk & below);
                if (keep && j < nCod) {
                        prot[j] = (uint8_t)aa;
                        kept[3 * j] = (uint8_t)r0; kept[3 * j + 1] = (uint8_t)r1; kept[3 * j + 2] = (uint8_t)r2;
                }
                run += __popcll(mk);
                stops += __popcll(__ballot(stop));
                xs += __popcll(__ballot(x));
        }
        const long long rec = lane == KA_COD_CODONS ? nCod : lane == KA_COD_STOPS ? stops : xs;
        if (lane >= KA_COD_CODONS && lane <= KA_COD_X) a.recs[i * KA_COD_DEVREC + lane] = (int)rec;
}

__global__ __launch_bounds__(KA_COD_THREADS) void cod_back(KaCodBackTab a)
{
        const int lane = threadIdx.x & 63;
        const long long r = (long long)blockIdx.x * (KA_COD_THREADS / 64) + (threadIdx.x >> 6);
        if (r >= a.nSeq) return;                                 // (the whole wave)
        const int f = ka_fam_find(a.famFirst, a.nFam, (int)r);
        const long long W = a.alnlen[f], p = r - a.famFirst[f];
        const uint8_t* in = a.rows + a.rowOff[f] + p * (W + 1);
        uint8_t* out = a.out + a.outOff[f] + p * (3 * W + 1);
        const uint8_t* kept = a.kept + a.seqOff[r];
        const long long nKept = a.recs[r * KA_COD_DEVREC + KA_COD_CODONS] - a.recs[r * KA_COD_DEVREC + KA_COD_STOPS];
        const int gap = a.gap;
        const unsigned long long below = ka_lanes_below(lane);
        long long run = 0;
        for (long long c0 = 0; c0 < W; c0 += KA_IN_STEP) {
                int b[KA_IN_STEP / 64];
                ka_walk_step<KA_IN_STEP>(in, W, c0, lane, b);
#pragma unroll
                for (int q = 0; q < KA_IN_STEP / 64; q++) {
                        const bool ch = b[q] >= 0 && b[q] != gap;
                        const unsigned long long m = __ballot(ch);
                        const long long j = c0 + 64 * q + lane, k = run + __popcll(m & below);
                        if (b[q] >= 0) {                         // (j < W)
                                const bool have = ch && k < nKept;
                                out[3 * j] = have ? kept[3 * k] : (uint8_t)gap;
                                out[3 * j + 1] = have ? kept[3 * k + 1] : (uint8_t)gap;
                                out[3 * j + 2] = have ? kept[3 * k + 2] : (uint8_t)gap;
                        }
                        run += __popcll(m);
                }
        }
        if (lane == 0) {
                out[3 * W] = 0;
                a.count[r] = (int)run;
        }
}

} // namespace

void ka_cod_run_pack(const KaCodTab& a, hipStream_t s, int* launches)
{
        cod_pack<<<ka_wave_grid(a.nSeq, KA_COD_THREADS), KA_COD_THREADS, 0, s>>>(a);
        ++*launches;
}

void ka_cod_run_translate(const KaCodTab& a, hipStream_t s, int* launches)
{
        cod_translate<<<ka_wave_grid(a.nSeq, KA_COD_THREADS), KA_COD_THREADS, 0, s>>>(a);
        ++*launches;
}

void ka_cod_run_back(const KaCodBackTab& a, hipStream_t s, int* launches)
{
        cod_back<<<ka_wave_grid(a.nSeq, KA_COD_THREADS), KA_COD_THREADS, 0, s>>>(a);
        ++*launches;
}
