// ka_cod.h -- the codon stage of a batch of families (ka_cod.hip kernels, ka_cod.cpp host side): what the two units share.
//
// The rule (include/kalign_amd.h, the codon stage; the reference's benchmarks/downstream/positive_selection.py:49-123): a
// sequence's residues by the input stage's byte rule (ka_in.h), upper-cased; three residues a codon; the standard code over
// exactly A C G T, X for a codon with any other letter (U is not T); stop codons omitted wherever they stand.
#pragma once
#include "ka_in.h"

#define KA_COD_THREADS 256         // every kernel: four waves, four sequences or rows, per workgroup
#define KA_COD_DEVREC 7            // a sequence's record from the device: see the enum below
#define KA_COD_SEQREC 6            // ... as ka_cod_fam_sequences hands it out: without KA_COD_BAD
#define KA_COD_STATS 9             // ka_cod_fam_stats: see include/kalign_amd.h

enum {
        KA_COD_RESIDUES = 0,       // letters
        KA_COD_GAPS = 1,           // punctuation
        KA_COD_DROPPED = 2,        // the other bytes below 128
        KA_COD_CODONS = 3,         // residues / 3
        KA_COD_STOPS = 4,          // TAA, TAG, TGA among them
        KA_COD_X = 5,              // codons with a letter outside A C G T
        KA_COD_BAD = 6,            // offset of the first byte >= 128 in the sequence's raw bytes, or -1
};

// index 16a + 4b + c with A 0, C 1, G 2, T 3
#define KA_COD_LETTERS "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"

// the 2-bit code of an upper-case letter, -1 outside A C G T
__host__ __device__ __forceinline__ int ka_cod_code(int b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1; }

// sequences are numbered flat over the batch in input order, family f's are famFirst[f] .. famFirst[f + 1] - 1.  The three
// planes are as large as the raw text; sequence i's part of each starts at seqOff[i] (there are never more residues than raw
// bytes, more amino acids than codons, or more kept codons than codons).
struct KaCodTab {
        int nSeq;
        const uint8_t* text;
        const long long* seqOff;               // [nSeq + 1]
        int* recs;                             // [nSeq][KA_COD_DEVREC]
        const uint8_t* table;                  // [64] KA_COD_LETTERS
        uint8_t* packed;                       // the pack: upper-cased residues
        uint8_t* protein;                      // the translate: amino-acid letters of the codons that are no stop
        uint8_t* kept;                         // ... and those codons' three bytes each
};

// protein rows in, codon rows out: family f's rows are alnlen[f] + 1 bytes apart from rowOff[f] on, its codon rows
// 3 * alnlen[f] + 1 bytes apart from outOff[f] on (each row ends in a 0 byte, as ka_batch_rows packs them)
struct KaCodBackTab {
        int nFam, nSeq, gap;
        const int* famFirst;                   // [nFam + 1]
        const int* alnlen;                     // [nFam]
        const long long* rowOff;               // [nFam]
        const long long* outOff;               // [nFam]
        const uint8_t* rows;
        const long long* seqOff;               // [nSeq + 1]
        const int* recs;                       // [nSeq][KA_COD_DEVREC]
        const uint8_t* kept;
        uint8_t* out;
        int* count;                            // [nSeq] non-gap bytes of each row
};

// ka_cod.hip: every launcher adds the kernels it launches to *launches
void ka_cod_run_pack(const KaCodTab& a, hipStream_t s, int* launches);
void ka_cod_run_translate(const KaCodTab& a, hipStream_t s, int* launches);
void ka_cod_run_back(const KaCodBackTab& a, hipStream_t s, int* launches);
