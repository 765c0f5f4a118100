// ka_in.h -- the input stage of a batch of families (ka_in.hip kernels, ka_in.cpp host side): what the two units share.
//
// The rule for a byte (include/kalign_amd.h, the input stage; the reference's msa_io.c:454-468 in the C locale): below 128 a
// letter is a residue and kept as given, punctuation is a gap character, everything else is dropped; a byte of 128 or more
// is an error, reported by its offset.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define KA_IN_STEP 256             // raw bytes per step of the walk along a sequence: four ballots of 64
#define KA_IN_SCAN_THREADS 1024    // in_scan: sixteen waves, sixteen consecutive sequences, per workgroup
#define KA_IN_ENC_THREADS 256      // in_encode: four waves, four sorted positions, per workgroup
#define KA_IN_BINS 128             // a family's histogram
#define KA_IN_DEVREC 5             // a sequence's record from the device: see the enum below
#define KA_IN_SEQREC 4             // ... as ka_in_fam_sequences hands it out: without KA_IN_BAD
#define KA_IN_FAMREC 5             // ka_in_fam_families' record: biotype, status, min and max residues, letters without a code
#define KA_IN_STATS 6              // ka_in_fam_stats: see include/kalign_amd.h
#define KA_IN_TABLES 3             // nucleotides, reduced protein, protein

enum {
        KA_IN_RESIDUES = 0,        // letters
        KA_IN_GAPS = 1,            // punctuation
        KA_IN_DROPPED = 2,         // the other bytes below 128
        KA_IN_CHECKSUM = 3,        // GCGchecksum of the residues as kept
        KA_IN_BAD = 4,             // offset of the first byte >= 128 in the sequence's raw bytes, or -1
};

__host__ __device__ __forceinline__ bool ka_in_is_letter(int b) { return (unsigned)((b | 32) - 'a') < 26u && b < 128; }
__host__ __device__ __forceinline__ bool ka_in_is_punct(int b)
{
        return (b >= 33 && b <= 47) || (b >= 58 && b <= 64) || (b >= 91 && b <= 96) || (b >= 123 && b <= 126);
}

// sequences are numbered flat over the batch, families in order: family f's are famFirst[f] .. famFirst[f + 1] - 1, in input
// order for the scan and in sorted order for the encode (a family's sorted positions are its own range)
struct KaInTab {
        int nFam, nSeq;
        const int* famFirst;                   // [nFam + 1]
        const uint8_t* text;
        const long long* seqOff;               // [nSeq + 1] raw bytes of sequence i: text[seqOff[i] .. seqOff[i + 1])
        // the scan
        int* recs;                             // [nSeq][KA_IN_DEVREC]
        unsigned long long* freq;              // [nFam][KA_IN_BINS] (zeroed first by the caller)
        // the encode
        const int* order;                      // [nSeq] sorted position -> input index
        const long long* outOff;               // [nSeq + 1] where the residues of a sorted position start in each plane
        const uint8_t* biotype;                // [nFam] 0 protein, 1 DNA
        const int8_t* tables;                  // [KA_IN_TABLES][128], -1: no code
        uint8_t* letters; uint8_t* treeCodes; uint8_t* codes;
        unsigned long long* noCode;            // [nFam] (zeroed first by the caller)
};

// ka_in.hip: every launcher adds the kernels it launches to *launches
void ka_in_run_scan(const KaInTab& a, hipStream_t s, int* launches);
void ka_in_run_encode(const KaInTab& a, hipStream_t s, int* launches);
