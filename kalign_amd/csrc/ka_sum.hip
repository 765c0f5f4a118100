// ka_sum.hip -- summaries and trimming of the finished rows of a batch of families on the device: one kernel set over
// tables of families (ka_sum.h); one alignment is a batch of one.  No launch count depends on the number of families.
//
//   sum_columns    a workgroup per tile of 64 columns of one family (the family found by ka_fam_find over the first-tile
//                  table): its waves deal the family's rows among them, a lane per column, and count bytes into a
//                  bin-major LDS histogram (256 bins x 64 columns: the lanes of a wave never share a counter); the bins
//                  are reduced in eight parts of 32, a wave each, then per column by the first wave: gaps, distinct
//                  characters, the most frequent character and its count, the sum of C(n_a, 2).  A tie for the highest
//                  count is settled as Counter.most_common does, by the first row that holds one of the tied characters: a
//                  second walk of the tied columns, dealt to the waves like the first, that ends at that row (an LDS
//                  minimum per column).  The family's four sums by 64-bit atomics, its character-presence mask by 32-bit
//                  ORs.
//   sum_consensus  flat over the columns of the batch
//   sum_keep       flat over the columns: the caller's mask or the gap-fraction rule
//   sum_scan       a workgroup per family: the kept columns numbered in order (256 columns a step, the count carried)
//   sum_offsets    one workgroup: where every family's compacted rows start
//   sum_gather     a wave per (row, chunk of 256 output columns): four consecutive output bytes per lane
//   sum_identity   the pairwise identity matrices: a workgroup per upper-triangle tile of 32 x 32 pairs of rows of one family
//                  (a table of tiles; the family by ka_fam_find over its first-tile table).  The width in chunks of 128
//                  columns staged in LDS with per-row character marks; a lane holds 2 x 2 pairs and takes four columns per
//                  32-bit operation: XOR, an exact zero-byte test, population counts.  Exact counts, the doubles one
//                  division each, both triangles written by the tile of the upper one.
//   sum_gap_rows   the walk along rows: a wave per row of the batch (the family by ka_fam_find over the first-row table), 256
//                  columns a step as four ballots of 64.  Per row its characters, leading and trailing gap columns and gap
//                  blocks from population counts, count-leading / count-trailing zeros and one carried bit; the record to
//                  memory, the family's four sums by 64-bit atomics, once per family that a workgroup of 16 rows meets.
//   sum_gappy      flat over the columns: the columns with 2 nGap > N of every family, from the column table
//   sum_ungap      a wave per row: its characters packed in order at the row's 64-bit offset, a lane's place the
//                  population count of the character mask below it
#include <algorithm>
#include "ka_sum.h"
#include "ka_msa.h"
#include "ka_walk.h"

namespace {

// what one part of the bins knows about a column
struct SumPart {
        int dist, k, mx, arg, nmx;             // distinct characters, characters, highest count, its lowest bin, bins that have it
        long long same;
};

// ... as it lies in LDS: five words per (part, column), word-major (the lanes of a wave on neighbouring words); dist, arg
// and nmx share a word (a part has 32 bins: dist and nmx reach 32, arg 255)
enum { PART_K = 0, PART_MX = 1, PART_PACKED = 2, PART_SAME_LO = 3, PART_SAME_HI = 4, PART_WORDS = 5 };
constexpr int kPartSlots = KA_SUM_PARTS * KA_SUM_TILE;

__device__ __forceinline__ void part_put(unsigned* part, int slot, const SumPart& p)
{
        part[PART_K * kPartSlots + slot] = (unsigned)p.k;
        part[PART_MX * kPartSlots + slot] = (unsigned)p.mx;
        part[PART_PACKED * kPartSlots + slot] = (unsigned)p.dist | (unsigned)p.arg << 8 | (unsigned)p.nmx << 16;
        part[PART_SAME_LO * kPartSlots + slot] = (unsigned)p.same;
        part[PART_SAME_HI * kPartSlots + slot] = (unsigned)(p.same >> 32);
}

__device__ __forceinline__ SumPart part_get(const unsigned* part, int slot)
{
        SumPart p;
        const unsigned w = part[PART_PACKED * kPartSlots + slot];
        p.k = (int)part[PART_K * kPartSlots + slot];
        p.mx = (int)part[PART_MX * kPartSlots + slot];
        p.dist = (int)(w & 255u); p.arg = (int)(w >> 8 & 255u); p.nmx = (int)(w >> 16);
        p.same = (long long)((unsigned long long)part[PART_SAME_HI * kPartSlots + slot] << 32 | part[PART_SAME_LO * kPartSlots + slot]);
        return p;
}

// histogram, parts, two ints per column: 76 288 bytes, so that two workgroups share a CU's 160 KiB
constexpr size_t kColumnsLds = sizeof(unsigned) * (KA_SUM_BINS * KA_SUM_TILE + PART_WORDS * kPartSlots + 2 * KA_SUM_TILE);
static_assert(2 * kColumnsLds <= 163840, "two column-table workgroups per CU");

__global__ __launch_bounds__(KA_SUM_THREADS) void sum_columns(KaSumTab a)
{
        extern __shared__ unsigned sum_lds[];
        unsigned* hist = sum_lds;                                // [bin][column of the tile]
        unsigned* part = sum_lds + KA_SUM_BINS * KA_SUM_TILE;
        const int tile = blockIdx.x;
        const int f = ka_fam_find(a.tileFirst, a.nFam, tile);
        const KaSumFam fam = a.fams[f];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int c = (tile - a.tileFirst[f]) * KA_SUM_TILE + lane;
        const unsigned gap = a.gap;
        const long long stride = (long long)fam.W + 1;
        const uint8_t* col = a.rows + fam.rowOff + c;           // (read only where c < W)
        int* firstRow = (int*)(part + PART_WORDS * kPartSlots);          // [column]: the row that settles a tie
        int* tieMx = firstRow + KA_SUM_TILE;                             // [column]: the highest count of a tied column, else 0
        for (int i = threadIdx.x; i < KA_SUM_BINS * KA_SUM_TILE; i += KA_SUM_THREADS) hist[i] = 0;
        if (threadIdx.x < KA_SUM_TILE) firstRow[threadIdx.x] = INT32_MAX;
        __syncthreads();
        if (c < fam.W) {
#pragma unroll 4
                for (int r = wave; r < fam.N; r += KA_SUM_PARTS) atomicAdd(&hist[(unsigned)col[r * stride] * KA_SUM_TILE + lane], 1u);
        }
        __syncthreads();
        {
                SumPart p{};
                unsigned present = 0;
                for (int q = 0; q < KA_SUM_BINS / KA_SUM_PARTS; q++) {
                        const unsigned b = wave * (KA_SUM_BINS / KA_SUM_PARTS) + q;
                        const int n = (int)hist[b * KA_SUM_TILE + lane];
                        if (b == gap || !n) continue;
                        p.dist++;
                        p.k += n;
                        p.same += (long long)n * (n - 1) / 2;
                        present |= 1u << q;
                        if (n > p.mx) { p.mx = n; p.arg = (int)b; p.nmx = 1; }
                        else if (n == p.mx) p.nmx++;
                }
                part_put(part, wave * KA_SUM_TILE + lane, p);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) present |= __shfl_xor(present, o, 64);
                if (lane == 0 && present) atomicOr(&a.present[(long long)f * 8 + wave], present);
        }
        __syncthreads();
        // the first wave adds the parts up and tells the others which columns are tied, and at which count
        int dist = 0, k = 0, mx = 0, ties = 0;
        unsigned top = gap;
        long long same = 0;
        if (wave == 0) {
                for (int w = 0; w < KA_SUM_PARTS; w++) {
                        const SumPart p = part_get(part, w * KA_SUM_TILE + lane);
                        dist += p.dist;
                        k += p.k;
                        same += p.same;
                        if (p.mx > mx) { mx = p.mx; top = (unsigned)p.arg; ties = p.nmx; }
                        else if (p.mx == mx && mx > 0) ties += p.nmx;
                }
                tieMx[lane] = ties > 1 ? mx : 0;
        }
        __syncthreads();
        // a tie: the first row that holds a character of the highest count.  Each wave walks its own rows and ends at its
        // first such row, or where another wave has found a lower one; the lowest row wins.
        const int tmx = tieMx[lane];
        if (tmx)
                for (int r = wave; r < fam.N && r < *(volatile int*)&firstRow[lane]; r += KA_SUM_PARTS) {
                        const unsigned b = col[r * stride];
                        if (b != gap && (int)hist[b * KA_SUM_TILE + lane] == tmx) { atomicMin(&firstRow[lane], r); break; }
                }
        __syncthreads();
        if (wave != 0) return;
        if (ties > 1) top = col[firstRow[lane] * stride];
        const int nGap = (int)hist[gap * KA_SUM_TILE + lane];    // (0 past the family's width: nothing was counted there)
        if (c < fam.W) {
                const long long g = (long long)fam.firstCol + c;
                a.nGap[g] = nGap;
                a.nDistinct[g] = dist;
                a.topChar[g] = (uint8_t)top;
                a.topCount[g] = mx;
                a.samePairs[g] = same;
        }
        const long long sums[KA_SUM_FAMSUMS] = { nGap, k > 0 && dist == 1, same, (long long)k * (k - 1) / 2 };
#pragma unroll
        for (int q = 0; q < KA_SUM_FAMSUMS; q++) {
                const long long v = ka_msa_wave_sum(sums[q]);
                if (lane == 0 && v) atomicAdd(&a.famSums[(long long)f * KA_SUM_FAMSUMS + q], (unsigned long long)v);
        }
}

__global__ __launch_bounds__(256) void sum_consensus(KaSumTab a)
{
        const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
        if (g >= a.cols) return;
        const int f = ka_fam_find(a.colFirst, a.nFam, (int)g);
        const KaSumFam fam = a.fams[f];
        const int k = fam.N - a.nGap[g];
        uint8_t ch = a.gap;
        if (k > 0) ch = (double)a.topCount[g] / (double)k >= a.thr[f] ? a.topChar[g] : a.ambiguous[f];
        uint8_t* o = a.out + g + f;                              // (a 0 byte after each family's row)
        o[0] = ch;
        if ((int)g - fam.firstCol == fam.W - 1) o[1] = 0;
}

__global__ __launch_bounds__(256) void sum_keep(KaSumTab a)
{
        const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
        if (g >= a.cols) return;
        const int f = ka_fam_find(a.colFirst, a.nFam, (int)g);
        const KaSumFam fam = a.fams[f];
        const long long mo = a.masks ? a.maskOff[f] : -1;
        a.keep[g] = mo >= 0 ? a.masks[mo + ((int)g - fam.firstCol)] != 0 : (double)a.nGap[g] / (double)fam.N < a.thr[f];
}

__global__ __launch_bounds__(KA_SUM_SCAN) void sum_scan(KaSumTab a)
{
        __shared__ int waveTot[KA_SUM_SCAN / 64];
        const int f = blockIdx.x;
        const KaSumFam fam = a.fams[f];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        int carry = 0;
        for (int c0 = 0; c0 < fam.W; c0 += KA_SUM_SCAN) {
                const int c = c0 + threadIdx.x;
                const bool kp = c < fam.W && a.keep[fam.firstCol + c] != 0;
                const unsigned long long m = __ballot(kp);
                if (lane == 0) waveTot[wave] = __popcll(m);
                __syncthreads();
                int before = 0, all = 0;
                for (int w = 0; w < KA_SUM_SCAN / 64; w++) {
                        if (w < wave) before += waveTot[w];
                        all += waveTot[w];
                }
                if (kp) a.src[fam.firstCol + carry + before + __popcll(m & ((1ull << lane) - 1ull))] = c;
                carry += all;
                __syncthreads();
        }
        if (threadIdx.x == 0) a.newW[f] = carry;
}

__global__ __launch_bounds__(256) void sum_offsets(KaSumTab a)
{
        __shared__ long long waveTot[4];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        long long carry = 0;
        for (int f0 = 0; f0 < a.nFam; f0 += 256) {
                const int f = f0 + threadIdx.x;
                const long long v = f < a.nFam ? (long long)a.fams[f].N * (a.newW[f] + 1) : 0;
                long long inc = v;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                        const long long t = __shfl_up(inc, o, 64);
                        if (lane >= o) inc += t;
                }
                if (lane == 63) waveTot[wave] = inc;
                __syncthreads();
                long long before = 0, all = 0;
                for (int w = 0; w < 4; w++) {
                        if (w < wave) before += waveTot[w];
                        all += waveTot[w];
                }
                if (f < a.nFam) a.outOff[f] = carry + before + inc - v;
                carry += all;
                __syncthreads();
        }
}

__global__ __launch_bounds__(256) void sum_gather(KaSumTab a)
{
        const int lane = threadIdx.x & 63;
        const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
        if (item >= a.nItems) return;
        const int f = ka_fam_find(a.itemFirst, a.nFam, (int)item);
        const KaSumFam fam = a.fams[f];
        const int local = (int)item - a.itemFirst[f];
        const int row = local / fam.chunks, chunk = local % fam.chunks;
        const int nw = a.newW[f];
        const int j0 = chunk * KA_SUM_CHUNK + lane * 4;
        if (j0 > nw) return;
        const uint8_t* in = a.rows + fam.rowOff + (long long)row * (fam.W + 1);
        uint8_t* o = a.out + a.outOff[f] + (long long)row * (nw + 1);
        const int* src = a.src + fam.firstCol;
#pragma unroll
        for (int q = 0; q < 4; q++) {
                const int j = j0 + q;
                if (j < nw) o[j] = in[src[j]];
                else if (j == nw) o[j] = 0;
        }
}

// ---- the identity matrices ----------------------------------------------------------------------------------------------
// A row's chunk in LDS: its bytes as they stand, four columns a word (0 past the row's width and in a row past the family),
// and beside them its marks, 0x80 in every byte that holds a character.  Rows lie kIdmRowWords words apart: a quarter of
// that is odd, so the 16-byte reads of 8 consecutive rows at one column start at 8 different multiples of 4 modulo 64 and
// never share a bank.  A wave's lanes are 8 x 8: lane & 7 picks the row on the i side, lane >> 3 on the j side.  In each of
// ds_read_b128's four groups of 16 lanes an i-side read has 8 distinct rows (each read by two lanes: a broadcast) and a
// j-side read 4 -- consecutive rows at one column, so distinct banks: no read of the loop has a bank conflict.
constexpr int kIdmRowWords = KA_SUM_IDM_CHUNK / 4 + 4;
constexpr int kIdmRows = 2 * KA_SUM_IDM_T;                         // the i side, then the j side (a diagonal tile: one side)
constexpr size_t kIdmLds = sizeof(unsigned) * 2 * kIdmRows * kIdmRowWords;      // bytes and marks: 18 432 bytes
static_assert(kIdmRowWords % 4 == 0 && (kIdmRowWords / 4) % 2 == 1, "consecutive rows' 16-byte reads fall into different banks");
static_assert(2 * kIdmLds <= 163840, "two identity workgroups per CU");
static_assert(KA_SUM_IDM_THREADS == 256 && KA_SUM_IDM_CHUNK % 16 == 0, "four waves of 8 x 8 lanes; whole 16-byte reads");
constexpr int kIdmAhead = 16;                                      // words a thread loads before it uses the first, while staging
struct __attribute__((aligned(4))) IdmTwo { unsigned lo, hi; };     // two aligned words of the upload (which starts on a word)

// one word of two rows: columns where both hold a character, and those of them where the bytes are equal.  x | t has bit 7
// of a byte set exactly when the byte of x is not 0: t's bit 7 says that the low seven bits are not 0 (0x7f + 0x7f does not
// carry into the next byte), x's own bit 7 the rest.  Exact for every byte value, 0x01 beside 0x00 and 0x80 included.
__device__ __forceinline__ void idm_word(unsigned xi, unsigned yi, unsigned xj, unsigned yj, int& m, int& c)
{
        const unsigned both = yi & yj;
        const unsigned x = xi ^ xj;
        const unsigned t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
        c += __popc(both);
        m += __popc(__builtin_amdgcn_bitop3_b32(both, x, t, 0x10));    // both & ~x & ~t in one operation
}

__global__ __launch_bounds__(KA_SUM_IDM_THREADS) void sum_identity(KaIdmTab a)
{
        constexpr int T = KA_SUM_IDM_T, RT = KA_SUM_IDM_RT, WORDS = KA_SUM_IDM_CHUNK / 4;
        extern __shared__ __attribute__((aligned(16))) unsigned idm_lds[];
        unsigned* dat = idm_lds;                                 // [row of the tile's two sides][kIdmRowWords]
        unsigned* mrk = idm_lds + kIdmRows * kIdmRowWords;
        const int tile = blockIdx.x;
        const int f = ka_fam_find(a.tileFirst, a.nFam, tile);
        const KaSumFam fam = a.fams[f];
        const unsigned packed = a.tiles[tile];
        const int i0 = (int)(packed >> 16) * T, j0 = (int)(packed & 0xffffu) * T;
        const bool diag = i0 == j0;                              // one side is staged, and the quarter below the diagonal idles
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int wi = wave >> 1, wj = wave & 1, ti = lane & 7, tj = lane >> 3;
        const bool idle = diag && wi > wj;                       // (the whole wave)
        const unsigned gap4 = a.gap * 0x01010101u;
        const long long stride = (long long)fam.W + 1;
        const int nStage = (diag ? T : 2 * T) * WORDS;
        const int ri = wi * 8 * RT + ti, rj = (diag ? 0 : T) + wj * 8 * RT + tj;    // this lane's first rows in LDS; the others 8 apart
        int m[RT][RT] = {}, c[RT][RT] = {};
        for (int c0 = 0; c0 < fam.W; c0 += KA_SUM_IDM_CHUNK) {
                // stage: neighbouring lanes take neighbouring words of one row.  A row starts at any byte, so a word's four
                // columns come from the two aligned words of the upload that hold them, shifted together -- where both lie
                // inside the upload; the few words at its very end are put together byte by byte, no byte past the end is
                // read.  The loads of kIdmAhead words go out before the first is used.
                for (int s0 = 0; s0 < nStage; s0 += KA_SUM_IDM_THREADS * kIdmAhead) {
                        IdmTwo w[kIdmAhead];
#pragma unroll
                        for (int u = 0; u < kIdmAhead; u++) {
                                const int idx = s0 + u * KA_SUM_IDM_THREADS + threadIdx.x;
                                const int row = idx / WORDS, col = c0 + 4 * (idx % WORDS);
                                const int gr = row < T ? i0 + row : j0 + row - T;
                                const long long al = (fam.rowOff + (long long)gr * stride + col) & ~3ll;
                                w[u] = IdmTwo{ 0, 0 };
                                if (idx < nStage && gr < fam.N && col < fam.W && al + 8 <= a.bytes) w[u] = *(const IdmTwo*)(a.rows + al);
                        }
#pragma unroll
                        for (int u = 0; u < kIdmAhead; u++) {
                                const int idx = s0 + u * KA_SUM_IDM_THREADS + threadIdx.x;
                                if (idx >= nStage) continue;
                                const int row = idx / WORDS, k = idx % WORDS, col = c0 + 4 * k;
                                const int gr = row < T ? i0 + row : j0 + row - T;
                                const int nb = gr < fam.N ? min(4, max(0, fam.W - col)) : 0;       // the word's columns inside the row
                                const unsigned keep = nb >= 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u;
                                const long long g = fam.rowOff + (long long)gr * stride + col;
                                unsigned d = __funnelshift_r(w[u].lo, w[u].hi, 8u * (unsigned)(g & 3));
                                if (nb > 0 && (g & ~3ll) + 8 > a.bytes) {                          // (the upload's last bytes)
                                        d = 0;
                                        for (int q = 0; q < nb; q++) d |= (unsigned)a.rows[g + q] << (8 * q);
                                }
                                d &= keep;
                                const unsigned x = d ^ gap4;                                     // a byte of x is 0 at a gap
                                dat[row * kIdmRowWords + k] = d;
                                mrk[row * kIdmRowWords + k] = (x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u & keep;
                        }
                }
                __syncthreads();
                if (!idle) {
                        const int nq = (min(KA_SUM_IDM_CHUNK, fam.W - c0) + 15) / 16;
                        for (int q = 0; q < nq; q++) {
                                uint4 xi[RT], yi[RT];
#pragma unroll
                                for (int u = 0; u < RT; u++) {
                                        xi[u] = *(const uint4*)(dat + (ri + 8 * u) * kIdmRowWords + 4 * q);
                                        yi[u] = *(const uint4*)(mrk + (ri + 8 * u) * kIdmRowWords + 4 * q);
                                }
#pragma unroll
                                for (int v = 0; v < RT; v++) {
                                        const uint4 xj = *(const uint4*)(dat + (rj + 8 * v) * kIdmRowWords + 4 * q);
                                        const uint4 yj = *(const uint4*)(mrk + (rj + 8 * v) * kIdmRowWords + 4 * q);
#pragma unroll
                                        for (int u = 0; u < RT; u++) {
                                                idm_word(xi[u].x, yi[u].x, xj.x, yj.x, m[u][v], c[u][v]);
                                                idm_word(xi[u].y, yi[u].y, xj.y, yj.y, m[u][v], c[u][v]);
                                                idm_word(xi[u].z, yi[u].z, xj.z, yj.z, m[u][v], c[u][v]);
                                                idm_word(xi[u].w, yi[u].w, xj.w, yj.w, m[u][v], c[u][v]);
                                        }
                                }
                        }
                }
                __syncthreads();
        }
        if (idle) return;
        const long long ent = a.entFirst[f];
#pragma unroll
        for (int u = 0; u < RT; u++)
#pragma unroll
                for (int v = 0; v < RT; v++) {
                        const int i = i0 + wi * 8 * RT + ti + 8 * u, j = j0 + wj * 8 * RT + tj + 8 * v;
                        if (i >= fam.N || j >= fam.N || i > j) continue;     // (i > j: in a diagonal tile only; its mirror writes it)
                        const double id = i == j ? 1.0 : c[u][v] > 0 ? (double)m[u][v] / (double)c[u][v] : 0.0;
                        const long long e = ent + (long long)i * fam.N + j, e2 = ent + (long long)j * fam.N + i;
                        a.matches[e] = m[u][v]; a.compared[e] = c[u][v]; a.identity[e] = id;
                        if (i != j) { a.matches[e2] = m[u][v]; a.compared[e2] = c[u][v]; a.identity[e2] = id; }
                }
}

// ---- the walk along rows ------------------------------------------------------------------------------------------------
// A wave per row, rows numbered flat over the batch (the family by ka_fam_find over the first-row table), KA_SUM_CHUNK
// columns a step (ka_walk.h, in int: a family holds fewer than 2^31 cells).  A lane at or past column W is neither a gap nor
// a character.
struct RowWalk {
        const uint8_t* row;
        int f, W;
};

__device__ __forceinline__ RowWalk row_walk(const KaGapTab& a, int r)
{
        RowWalk w;
        w.f = ka_fam_find(a.rowFirst, a.nFam, r);
        const KaSumFam fam = a.fams[w.f];
        w.W = fam.W;
        w.row = a.rows + fam.rowOff + (long long)(r - a.rowFirst[w.f]) * ((long long)fam.W + 1);
        return w;
}

// A row's record and its share of the family's sums.  Gap blocks: a block starts at a gap whose left neighbour is no gap --
// inside a ballot the mask shifted by one, at its first column the carried bit, which says whether the last column of the
// ballot before was a gap (so a block that crosses an edge is counted once, and one that ends at an edge is counted).  The
// first and the last character of the row give leading and trailing; a row without a character has leading = trailing = W.
// The four sums of a workgroup's rows are folded into the families' (ka_fold_families: a family of thousands of rows would
// otherwise queue one atomic per row on the same four addresses).
__global__ __launch_bounds__(KA_SUM_GAP_THREADS) void sum_gap_rows(KaGapTab a)
{
        constexpr int kWaves = KA_SUM_GAP_THREADS / 64;
        __shared__ long long part[kWaves][KA_SUM_ROWREC];
        __shared__ int famOf[kWaves];                            // -1: no row
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const long long r = (long long)blockIdx.x * kWaves + wave;
        int f = -1;
        long long sum = 0;
        if (r < a.nRows) {                                       // (the whole wave)
                const RowWalk w = row_walk(a, (int)r);
                const int gap = a.gap;
                int gaps = 0, blocks = 0, first = w.W, last = -1;        // first, last: the columns of the first and last character
                unsigned long long carry = 0;
                for (int c0 = 0; c0 < w.W; c0 += KA_SUM_CHUNK) {
                        int b[KA_SUM_CHUNK / 64];
                        ka_walk_step<KA_SUM_CHUNK>(w.row, w.W, c0, lane, b);
#pragma unroll
                        for (int q = 0; q < KA_SUM_CHUNK / 64; q++) {
                                const unsigned long long m = __ballot(b[q] == gap), k = __ballot(b[q] >= 0 && b[q] != gap);
                                gaps += __popcll(m);
                                blocks += __popcll(m & ~(m << 1 | carry));
                                carry = m >> 63;                 // (read again only when this ballot was full)
                                if (k) {
                                        if (first == w.W) first = c0 + 64 * q + __ffsll((long long)k) - 1;
                                        last = c0 + 64 * q + 63 - __clzll((long long)k);
                                }
                        }
                }
                const int chars = w.W - gaps, leading = first, trailing = last < 0 ? w.W : w.W - 1 - last;
                const long long terminal = (long long)leading + trailing;
                const int rec = lane == KA_ROW_CHARS ? chars : lane == KA_ROW_LEADING ? leading : lane == KA_ROW_TRAILING ? trailing : blocks;
                sum = lane == KA_GAP_CHARS ? chars : lane == KA_GAP_BLOCKS ? blocks : lane == KA_GAP_TERMINAL ? terminal : max(0ll, gaps - terminal);
                static_assert(KA_SUM_ROWREC == 4 && KA_GAP_INTERNAL == 3, "four lanes write the record and hold the four row sums");
                if (lane < KA_SUM_ROWREC) a.recs[r * KA_SUM_ROWREC + lane] = rec;
                f = w.f;
        }
        if (lane < KA_SUM_ROWREC) part[wave][lane] = sum;
        if (lane == 0) famOf[wave] = f;
        __syncthreads();
        if (threadIdx.x < KA_SUM_ROWREC) ka_fold_families(part, famOf, threadIdx.x, a.sums, KA_SUM_GAPSUMS);
}

// flat over the columns of the batch: a column is gappy when more than half of its family's rows hold a gap, 2 nGap > N.
// A wave whose columns lie in one family adds their number once; where a family ends inside it, each gappy column adds for
// itself.
__global__ __launch_bounds__(256) void sum_gappy(KaGapTab a)
{
        const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
        const int lane = threadIdx.x & 63;
        int f = -1;
        bool gappy = false;
        if (g < a.cols) {
                f = ka_fam_find(a.colFirst, a.nFam, (int)g);
                gappy = 2ll * a.nGap[g] > a.fams[f].N;
        }
        const int f0 = __shfl(f, 0, 64);
        if (f0 < 0) return;                                      // (the whole wave is past the last column)
        unsigned long long* sums = a.sums + KA_GAP_GAPPY;
        if (__all(f == f0 || f < 0)) {
                const unsigned long long m = __ballot(gappy);
                if (lane == 0 && m) atomicAdd(&sums[(long long)f0 * KA_SUM_GAPSUMS], (unsigned long long)__popcll(m));
        } else if (gappy)
                atomicAdd(&sums[(long long)f * KA_SUM_GAPSUMS], 1ull);
}

// the characters of a row in order from out + off[r]: within a ballot a lane's place is the population count of the
// character mask below it, after the characters of the ballots before.  A wave reads and writes consecutive bytes.  The
// offsets come from the row records of sum_gap_rows, which applies the same rule to the same bytes; a write is held inside
// the row's own range regardless.
__global__ __launch_bounds__(KA_SUM_ROW_THREADS) void sum_ungap(KaGapTab a)
{
        const int lane = threadIdx.x & 63;
        const long long r = (long long)blockIdx.x * (KA_SUM_ROW_THREADS / 64) + (threadIdx.x >> 6);
        if (r >= a.nRows) return;
        const long long n = a.off[r + 1] - a.off[r];
        if (n <= 0) return;                                      // (an all-gap row)
        const RowWalk w = row_walk(a, (int)r);
        const int gap = a.gap;
        const unsigned long long below = ka_lanes_below(lane);
        uint8_t* o = a.out + a.off[r];
        long long run = 0;
        for (int c0 = 0; c0 < w.W && run < n; c0 += KA_SUM_CHUNK) {
                int b[KA_SUM_CHUNK / 64];
                ka_walk_step<KA_SUM_CHUNK>(w.row, w.W, c0, lane, b);
#pragma unroll
                for (int q = 0; q < KA_SUM_CHUNK / 64; q++) {
                        const bool ch = b[q] >= 0 && b[q] != gap;
                        const unsigned long long k = __ballot(ch);
                        const long long j = run + __popcll(k & below);
                        if (ch && j < n) o[j] = (uint8_t)b[q];
                        run += __popcll(k);
                }
        }
}

} // namespace

// Each launcher counts its launches where it makes them (*launches is the caller's counter of the call).

int ka_sum_run_columns(const KaSumTab& a, hipStream_t s, int* launches)
{
        static_assert(KA_SUM_BINS / KA_SUM_PARTS == 32, "a part of the bins is one word of the presence mask");
        if (hipFuncSetAttribute((const void*)sum_columns, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kColumnsLds) != hipSuccess) return 1;
        sum_columns<<<(unsigned)a.nTiles, KA_SUM_THREADS, kColumnsLds, s>>>(a);
        ++*launches;
        return 0;
}

void ka_sum_run_consensus(const KaSumTab& a, hipStream_t s, int* launches)
{
        sum_consensus<<<(unsigned)(((long long)a.cols + 255) / 256), 256, 0, s>>>(a);
        ++*launches;
}

void ka_sum_run_keep(const KaSumTab& a, hipStream_t s, int* launches)
{
        sum_keep<<<(unsigned)(((long long)a.cols + 255) / 256), 256, 0, s>>>(a);
        ++*launches;
        sum_scan<<<(unsigned)a.nFam, KA_SUM_SCAN, 0, s>>>(a);
        ++*launches;
}

void ka_sum_run_gather(const KaSumTab& a, hipStream_t s, int* launches)
{
        sum_offsets<<<1, 256, 0, s>>>(a);
        ++*launches;
        sum_gather<<<ka_wave_grid(a.nItems, 256), 256, 0, s>>>(a);
        ++*launches;
}

void ka_sum_run_gaps(const KaGapTab& a, hipStream_t s, int* launches)
{
        sum_gap_rows<<<ka_wave_grid(a.nRows, KA_SUM_GAP_THREADS), KA_SUM_GAP_THREADS, 0, s>>>(a);
        ++*launches;
        sum_gappy<<<(unsigned)(((long long)a.cols + 255) / 256), 256, 0, s>>>(a);
        ++*launches;
}

void ka_sum_run_ungap(const KaGapTab& a, hipStream_t s, int* launches)
{
        sum_ungap<<<ka_wave_grid(a.nRows, KA_SUM_ROW_THREADS), KA_SUM_ROW_THREADS, 0, s>>>(a);
        ++*launches;
}

int ka_sum_run_identity(const KaIdmTab& a, hipStream_t s, int* launches)
{
        if (hipFuncSetAttribute((const void*)sum_identity, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kIdmLds) != hipSuccess) return 1;
        sum_identity<<<(unsigned)a.nTiles, KA_SUM_IDM_THREADS, kIdmLds, s>>>(a);
        ++*launches;
        return 0;
}
