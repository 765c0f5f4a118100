// ka_out.h -- the output stage of a batch of families (ka_out.hip kernels, ka_out.cpp host side): what the two units share.
//
// The rule for a byte of a row is ka_sum.h's: a gap is the byte `gap`, every other byte is a character.  A text is made of
// lines, and every line of every format has one shape:
//     [pre] [label, padded with spaces to labelW] [mid] [body: cols bytes] '\n'
// so a byte of the text is a pure function of its offset: the family (a search over famOff), the line (closed forms over
// the family's record, ka_out_locate below), the place in the line (ka_out.hip: out_fetch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define KA_OUT_BLOCK 60            // columns of a Clustal / MSF block, and the reference's FASTA line
#define KA_OUT_NAME_PAD 5          // a block line's name is padded to the family's longest name + 5
#define KA_OUT_NAME_MAX 255        // bytes of a name (MSA_NAME_LEN is 256 with the terminator)
#define KA_OUT_STEP 256            // columns per step of the MSF row pass: four per lane, as KA_SUM_CHUNK
#define KA_OUT_ROW_THREADS 256     // out_rows: four waves, four rows, per workgroup
#define KA_OUT_FILL_THREADS 256    // out_fill: a lane per aligned dword of the text
#define KA_OUT_STATS 4             // ka_out_fam_stats: see include/kalign_amd.h
#define KA_OUT_NONE (~0ull)        // the offender record while nothing offends

enum { KA_OUT_FASTA = 0, KA_OUT_BLOCKS = 1, KA_OUT_STOCKHOLM = 2 };   // (Clustal and MSF differ in their headers alone)
enum { KA_OUT_PRE_NONE = 0, KA_OUT_PRE_FASTA = 1, KA_OUT_PRE_GR = 2, KA_OUT_PRE_GC = 3, KA_OUT_PRE_END = 4 };   // "", ">", "#=GR ", "#=GC ", "//"
enum { KA_OUT_MID_NONE = 0, KA_OUT_MID_ROW = 1, KA_OUT_MID_PP = 2 };                                            // "", "   ", " PP "
enum { KA_OUT_BODY_BYTES = 0, KA_OUT_BODY_PP = 1, KA_OUT_BODY_PPCONS = 2, KA_OUT_BODY_HDR = 3 };

// one family: N rows of W columns from rows + rowOff, W + 1 bytes apart; its rows are firstRow .. firstRow + N - 1 of the
// batch, its longest name holds nameMax bytes.  The rest is a call's: where its text starts and its header lies.
struct KaOutFam {
        int N, W;
        int firstRow, nameMax;
        long long rowOff;
        long long hdrOff;                      // of its header in `hdr`
        int hdrLen;                            // bytes of the header, the last '\n' included (0: none)
        int pad;
        long long confOff;                     // of its residue confidences (N * W floats)
        long long colOff;                      // of its column confidences (W floats)
        long long keyBase;                     // of its confidences in the offender record's order: (N + 1) W keys a family
};

struct KaOutTab {
        int nFam, nRows;
        int format;                            // KA_OUT_FASTA, KA_OUT_BLOCKS, KA_OUT_STOCKHOLM
        int lineLength;                        // FASTA
        int hasRes, hasCol;                    // Stockholm
        uint8_t gap;
        long long total;                       // bytes of the text; the buffer holds the next multiple of four
        const KaOutFam* fams;                  // [nFam]
        const long long* famOff;               // [nFam + 1] where a family's text starts
        const long long* rowOut;               // [nRows + 1] FASTA: where a row's text starts
        const int* rowFirst;                   // [nFam + 1]
        const uint8_t* rows;
        const uint8_t* names; const long long* nameOff;   // [nRows + 1]
        const uint8_t* hdr;
        const float* resConf; const float* colConf;
        unsigned long long* offender;          // the lowest key of a confidence outside [0, 1]
        int* recs;                             // [nRows][2] the MSF row pass: characters, prefix checksum
        uint8_t* out;
};

// one line of a text
struct KaOutLine {
        long long begin;                       // offset of its first byte in the text
        int pre, mid, body;
        int labelLen, labelW;
        long long cols;
        const uint8_t* label;
        const uint8_t* src;                    // body bytes: row bytes, or the header
        const float* conf;                     // PP: the confidences of these columns
        long long key;                         // ... and the key of the first
};

__host__ __device__ __forceinline__ int ka_out_pre_len(int pre) { return pre == KA_OUT_PRE_NONE ? 0 : pre == KA_OUT_PRE_FASTA ? 1 : pre == KA_OUT_PRE_END ? 2 : 5; }
__host__ __device__ __forceinline__ int ka_out_mid_len(int mid) { return mid == KA_OUT_MID_NONE ? 0 : mid == KA_OUT_MID_ROW ? 3 : 4; }
__host__ __device__ __forceinline__ long long ka_out_line_len(const KaOutLine& l)
{
        return ka_out_pre_len(l.pre) + l.labelW + ka_out_mid_len(l.mid) + l.cols + 1;
}

// The PP byte of a confidence (kalign.io._conf_to_pp_char on the float's value as a double), or -1 for a NaN and a value
// outside [0, 1].  -0.0 is 0.  The one place this rule lives: the kernel and ka_out_pp_char both call it.
__host__ __device__ __forceinline__ int ka_out_pp(float f)
{
        const double v = (double)f;
        if (!(v >= 0.0 && v <= 1.0)) return -1;
        if (v >= 0.95) return '*';
        return '0' + (int)(v * 10.0);
}

// the lengths the host's closed forms and the kernel's walk share
__host__ __device__ __forceinline__ long long ka_out_blocks(int W) { return ((long long)W + KA_OUT_BLOCK - 1) / KA_OUT_BLOCK; }
__host__ __device__ __forceinline__ long long ka_out_block_stride(const KaOutFam& d)    // a full block: N lines and the two newlines
{
        return (long long)d.N * (d.nameMax + KA_OUT_NAME_PAD + KA_OUT_BLOCK + 1) + 2;
}
__host__ __device__ __forceinline__ long long ka_out_sto_row_len(const KaOutFam& d) { return (long long)d.nameMax + 3 + d.W + 1; }
__host__ __device__ __forceinline__ long long ka_out_sto_gr_len(const KaOutFam& d) { return 5ll + d.nameMax + 4 + d.W + 1; }
__host__ __device__ __forceinline__ long long ka_out_sto_gc_len(const KaOutFam& d) { return 5ll + (d.nameMax > 7 ? d.nameMax : 7) + 3 + d.W + 1; }

// ka_out.hip: every launcher adds the kernels it launches to *launches
void ka_out_run_rows(const KaOutTab& a, hipStream_t s, int* launches);       // the MSF row pass: recs
void ka_out_run_fill(const KaOutTab& a, hipStream_t s, int* launches);       // the text of the batch in a.format
