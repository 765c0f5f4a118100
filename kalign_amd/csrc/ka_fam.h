// ka_fam.h -- what the stages of a batch of families share on the host: the family table's rule, the words that name a
// sequence of a family, the size of a packed batch of rows, and the checks one stage lends another.  The standard library
// and fail() alone: a stand-alone program links a stage's host-only build (-DKA_IN_HOST_ONLY, -DKA_COD_HOST_ONLY) with a
// fail() of its own and no HIP runtime.
#pragma once
#include <stdint.h>
#include <string>

#include "kalign_amd.h"

#ifndef KA_INTERNAL
#define KA_INTERNAL __attribute__((visibility("hidden")))
#endif
// the thread's error text (ka_last_error) and the one way to set it: ka_api.cpp, or the stand-alone program
KA_INTERNAL int fail(const std::string& m);

// The family table: sequences (or rows) are numbered flat over the batch, family f's are fam_first[f] .. fam_first[f + 1] - 1.
// fam_first ascends from 0 to numseq and no family is empty.  The one statement of the rule; errors read "<me>: ...".
inline int ka_fam_check_first(const std::string& me, int n_fam, const int* fam_first)
{
        if (n_fam < 1 || !fam_first) return fail(me + ": bad arguments");
        if (fam_first[0] != 0) return fail(me + ": fam_first does not ascend from 0 to numseq");
        for (int f = 0; f < n_fam; f++) {
                if (fam_first[f + 1] < fam_first[f]) return fail(me + ": fam_first does not ascend from 0 to numseq");
                if (fam_first[f + 1] == fam_first[f]) return fail(me + ": empty family");
        }
        return KA_OK;
}

// "<me>: family f, sequence i" (i: the sequence's number inside its family)
inline std::string ka_fam_where(const std::string& me, int f, int i)
{
        return me + ": family " + std::to_string(f) + ", sequence " + std::to_string(i);
}

// the bytes of a batch of rows packed as ka_batch_rows packs them: family f's N rows of alnlens[f] columns, alnlens[f] + 1
// bytes each
inline long long ka_fam_row_bytes(int n_fam, const int* fam_first, const int* alnlens)
{
        long long bytes = 0;
        for (int f = 0; f < n_fam; f++) bytes += (long long)(fam_first[f + 1] - fam_first[f]) * ((long long)alnlens[f] + 1);
        return bytes;
}

// a stage's check under another stage's name: ka_in_fam_check's rules (ka_in.cpp; the codon stage), ka_sum_fam_check's
// (ka_sum.cpp; the output stage)
int ka_in_check_named(const std::string& me, int n_fam, const int* fam_first, const long long* seq_off, long long n_bytes);
int ka_sum_check_named(const std::string& me, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens);
