// ka_out.hip -- the kernels of the output stage (gfx950, wave64): the finished rows of a batch of families -> alignment text.
//   out_rows    the MSF row pass: a wave per row, four rows per workgroup, KA_OUT_STEP columns a step, consecutive lanes on
//               consecutive columns.  First the row's characters (ballots over its whole width), then the checksum of the
//               prefix of that many BYTES of the aligned row, gaps included: the lanes' terms (column % 57 + 1) * upper-case
//               byte are summed in 64-bit integers and reduced % 10000 once (fewer than 2^31 terms below 2^14 each; the
//               remainder of the sum is what the reference's running remainder comes to).  The weight's index is the column,
//               so a lane takes column % 57 of its own column and no step needs the one before it.
//   out_fill    every format: a lane per aligned dword of the text, consecutive lanes on consecutive dwords, so a wave
//               stores 256 consecutive bytes whatever lines they fall into.  A lane finds the line its first byte lies in
//               (out_locate: a search over the families' offsets, then closed forms), fetches its four bytes (out_fetch) --
//               finding the next line when one ends inside the dword, so a dword is assembled from as many lines as it
//               spans -- and stores one dword.  The buffer holds a multiple of four bytes; the bytes past the text are 0.
//               No atomics, no scan, but for the offender record: a confidence outside [0, 1] sends its key (its place in
//               batch order) through one 64-bit atomicMin, so the lowest key stands whatever the scheduling.
// All stores are plain C++ stores of the vector unit.
#include "ka_out.h"
#include "ka_msa.h"          // ka_fam_find
#include "ka_walk.h"         // ka_wave_sum, ka_wave_grid (the row pass reads a prefix, not a row: its loads are its own)

namespace {

static_assert(KA_OUT_STEP == KA_WALK_STEP, "the row pass takes the walk's step");

__global__ __launch_bounds__(KA_OUT_ROW_THREADS) void out_rows(KaOutTab a)
{
        const int lane = threadIdx.x & 63;
        const long long r = (long long)blockIdx.x * (KA_OUT_ROW_THREADS / 64) + (threadIdx.x >> 6);
        if (r >= a.nRows) return;                                // (the whole wave)
        const int f = ka_fam_find(a.rowFirst, a.nFam, (int)r);
        const KaOutFam d = a.fams[f];
        const uint8_t* row = a.rows + d.rowOff + (r - d.firstRow) * ((long long)d.W + 1);
        const long long W = d.W;
        long long chars = 0;
        for (long long c0 = 0; c0 < W; c0 += KA_OUT_STEP) {
#pragma unroll
                for (int q = 0; q < KA_OUT_STEP / 64; q++) {
                        const long long c = c0 + 64 * q + lane;
                        chars += __popcll(__ballot(c < W && row[c] != a.gap));
                }
        }
        long long chk = 0;
        for (long long c0 = 0; c0 < chars; c0 += KA_OUT_STEP) {  // (chars <= W: the prefix lies inside the row)
#pragma unroll
                for (int q = 0; q < KA_OUT_STEP / 64; q++) {
                        const long long c = c0 + 64 * q + lane;
                        if (c >= chars) continue;
                        const int b = row[c];
                        chk += (c % 57 + 1) * (long long)(b >= 'a' && b <= 'z' ? b - 32 : b);
                }
        }
        chk = ka_wave_sum(chk) % 10000;
        if (lane == 0) {
                a.recs[2 * r] = (int)chars;
                a.recs[2 * r + 1] = (int)chk;
        }
}

// the last k of lo .. hi with first[k] <= x (first[lo] <= x)
__device__ __forceinline__ int out_find(const long long* first, int lo, int hi, long long x)
{
        while (lo < hi) {
                const int mid = (int)(((long long)lo + hi + 1) >> 1);
                if (first[mid] <= x) lo = mid;
                else hi = mid - 1;
        }
        return lo;
}

// the line byte o of the text lies in (0 <= o < a.total)
__device__ KaOutLine out_locate(const KaOutTab& a, long long o)
{
        KaOutLine l{};
        if (a.format == KA_OUT_FASTA) {
                const int r = out_find(a.rowOut, 0, a.nRows - 1, o);
                const KaOutFam& d = a.fams[ka_fam_find(a.rowFirst, a.nFam, r)];
                const long long n0 = a.nameOff[r], at = a.rowOut[r];
                const int nl = (int)(a.nameOff[r + 1] - n0);
                long long p = o - at;
                if (p < nl + 2) {                                // ">name\n"
                        l.begin = at; l.pre = KA_OUT_PRE_FASTA; l.label = a.names + n0; l.labelLen = l.labelW = nl;
                        return l;
                }
                p -= nl + 2;
                const long long L = a.lineLength, q = p / (L + 1);
                l.begin = at + nl + 2 + q * (L + 1);
                l.cols = d.W - q * L < L ? d.W - q * L : L;
                l.src = a.rows + d.rowOff + (long long)(r - d.firstRow) * ((long long)d.W + 1) + q * L;
                return l;
        }
        const int f = out_find(a.famOff, 0, a.nFam - 1, o);
        const KaOutFam& d = a.fams[f];
        long long p = o - a.famOff[f];
        if (p < d.hdrLen) {                                      // the header, its last '\n' the line's own
                l.begin = a.famOff[f]; l.body = KA_OUT_BODY_HDR; l.cols = d.hdrLen - 1; l.src = a.hdr + d.hdrOff;
                return l;
        }
        p -= d.hdrLen;
        const long long base = a.famOff[f] + d.hdrLen;
        if (a.format == KA_OUT_BLOCKS) {
                const long long nb = ka_out_blocks(d.W), stride = ka_out_block_stride(d);
                long long b = p / stride;
                if (b > nb - 1) b = nb - 1;                      // (the last block's two newlines)
                p -= b * stride;
                const long long cols = d.W - KA_OUT_BLOCK * b < KA_OUT_BLOCK ? d.W - KA_OUT_BLOCK * b : KA_OUT_BLOCK;
                const long long len = d.nameMax + KA_OUT_NAME_PAD + cols + 1, r = p / len;
                if (r >= d.N) {                                  // one of the two newlines after a block: an empty line each
                        l.begin = base + b * stride + p;
                        return l;
                }
                const long long n0 = a.nameOff[d.firstRow + r];
                l.begin = base + b * stride + r * len;
                l.label = a.names + n0; l.labelLen = (int)(a.nameOff[d.firstRow + r + 1] - n0); l.labelW = d.nameMax + KA_OUT_NAME_PAD;
                l.cols = cols;
                l.src = a.rows + d.rowOff + r * ((long long)d.W + 1) + KA_OUT_BLOCK * b;
                return l;
        }
        // Stockholm
        const long long rowLen = ka_out_sto_row_len(d), stride = rowLen + (a.hasRes ? ka_out_sto_gr_len(d) : 0), r = p / stride;
        if (r < d.N) {
                const long long n0 = a.nameOff[d.firstRow + r];
                p -= r * stride;
                l.label = a.names + n0; l.labelLen = (int)(a.nameOff[d.firstRow + r + 1] - n0); l.labelW = d.nameMax;
                l.cols = d.W;
                l.src = a.rows + d.rowOff + r * ((long long)d.W + 1);
                if (p < rowLen) {                                // "name   row"
                        l.begin = base + r * stride; l.mid = KA_OUT_MID_ROW;
                } else {                                         // "#=GR name PP pp"
                        l.begin = base + r * stride + rowLen; l.pre = KA_OUT_PRE_GR; l.mid = KA_OUT_MID_PP; l.body = KA_OUT_BODY_PP;
                        l.conf = a.resConf + d.confOff + r * d.W; l.key = d.keyBase + r * d.W;
                }
                return l;
        }
        p -= (long long)d.N * stride;
        l.begin = base + (long long)d.N * stride;
        if (a.hasCol && p < ka_out_sto_gc_len(d)) {              // "#=GC PP_cons   pp" (label NULL: the constant)
                l.pre = KA_OUT_PRE_GC; l.labelLen = 7; l.labelW = d.nameMax > 7 ? d.nameMax : 7; l.mid = KA_OUT_MID_ROW; l.body = KA_OUT_BODY_PPCONS;
                l.cols = d.W; l.conf = a.colConf + d.colOff; l.key = d.keyBase + (long long)d.N * d.W;
                return l;
        }
        if (a.hasCol) l.begin += ka_out_sto_gc_len(d);
        l.pre = KA_OUT_PRE_END;                                  // "//"
        return l;
}

// byte pos of a line (0 <= pos < ka_out_line_len(l))
__device__ unsigned out_fetch(const KaOutTab& a, const KaOutLine& l, long long pos)
{
        int k = ka_out_pre_len(l.pre);
        if (pos < k) return l.pre == KA_OUT_PRE_FASTA ? '>' : l.pre == KA_OUT_PRE_END ? '/' : l.pre == KA_OUT_PRE_GR ? "#=GR "[pos] : "#=GC "[pos];
        pos -= k;
        if (pos < l.labelW) return pos >= l.labelLen ? ' ' : l.label ? l.label[pos] : "PP_cons"[pos];
        pos -= l.labelW;
        k = ka_out_mid_len(l.mid);
        if (pos < k) return l.mid == KA_OUT_MID_PP ? " PP "[pos] : ' ';
        pos -= k;
        if (pos >= l.cols) return '\n';
        if (l.body == KA_OUT_BODY_BYTES || l.body == KA_OUT_BODY_HDR) return l.src[pos];
        if (l.body == KA_OUT_BODY_PP && (l.src[pos] == '-' || l.src[pos] == '.')) return '.';   // (the reference's test, not the handle's gap)
        const int c = ka_out_pp(l.conf[pos]);
        if (c >= 0) return (unsigned)c;
        atomicMin(a.offender, (unsigned long long)(l.key + pos));
        return '?';                                              // (the host hands no text out)
}

__global__ __launch_bounds__(KA_OUT_FILL_THREADS) void out_fill(KaOutTab a)
{
        const long long w = (long long)blockIdx.x * KA_OUT_FILL_THREADS + threadIdx.x, o = 4 * w;
        if (o >= a.total) return;
        KaOutLine l = out_locate(a, o);
        long long end = l.begin + ka_out_line_len(l);
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
                const long long x = o + k;
                if (x >= a.total) break;
                if (x >= end) {
                        l = out_locate(a, x);
                        end = l.begin + ka_out_line_len(l);
                }
                word |= (out_fetch(a, l, x - l.begin) & 255u) << (8 * k);
        }
        reinterpret_cast<unsigned*>(a.out)[w] = word;
}

} // namespace

void ka_out_run_rows(const KaOutTab& a, hipStream_t s, int* launches)
{
        out_rows<<<ka_wave_grid(a.nRows, KA_OUT_ROW_THREADS), KA_OUT_ROW_THREADS, 0, s>>>(a);
        ++*launches;
}

void ka_out_run_fill(const KaOutTab& a, hipStream_t s, int* launches)
{
        const long long words = (a.total + 3) / 4;               // (the host has refused a text of more than 2^39 bytes)
        out_fill<<<(unsigned)((words + KA_OUT_FILL_THREADS - 1) / KA_OUT_FILL_THREADS), KA_OUT_FILL_THREADS, 0, s>>>(a);
        ++*launches;
}
