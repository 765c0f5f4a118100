/*
 * ref_split_harness.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference's split2 (lib/src/bisectingKmeans.c:766-971) is `static`.  This translation unit is compiled by
 * oracle/Makefile (target `ref`, REF_CFLAGS: AVX2 edist_256, no FMA) into oracle/_ref/libkalign_ref.so: it includes the
 * reference's file BY NAME where it lies, with the four external functions of that file renamed so that they do not
 * collide with the ones libkalign_ref.so already holds, and wraps the real split2 for oracle/refdrv.py.  Nothing here
 * restates the algorithm.
 */
#define build_tree_kmeans        refh_split_unit_build_tree_kmeans
#define build_tree_kmeans_noisy  refh_split_unit_build_tree_kmeans_noisy
#define build_tree_from_pairwise refh_split_unit_build_tree_from_pairwise
#define upgma                    refh_split_unit_upgma
#include "bisectingKmeans.c"
#undef build_tree_kmeans
#undef build_tree_kmeans_noisy
#undef build_tree_from_pairwise
#undef upgma

#include <stdlib.h>
#include <string.h>

/* dm: numrows x padded floats, row-major, padded = num_anchors rounded up to a multiple of 8 (the columns beyond the
   anchors zero, as d_estimation leaves them).  samples[num_samples] index its rows.
   A whole candidate set at once (the seeds k * step, k < tries, of bisecting_kmeans :296-340), so that the matrix is
   copied once: score[tries], nlr[2 * tries] = nl, nr, lists[tries][2][num_samples] (sl then sr of every candidate).
   Returns 0, or 1 on failure. */
int refh_split_all(const float* dm, int numrows, int num_anchors, const int* samples, int num_samples, int tries, int step,
                   float* score, int* nlr, int* lists)
{
        const int padded = ((num_anchors + 7) / 8) * 8;
        float* flat = NULL;                     /* edist_256 loads rows with _mm256_load_ps: 32-byte aligned rows */
        const float** rows = NULL;
        int rc = 1;
        if(numrows < 1 || num_samples < 1 || tries < 1 || step < 0 || (long long)(tries - 1) * step >= num_samples) return 1;
        for(int i = 0; i < num_samples; i++) if(samples[i] < 0 || samples[i] >= numrows) return 1;
        if(posix_memalign((void**)&flat, 32, sizeof(float) * (size_t)numrows * padded)) return 1;
        rows = malloc(sizeof(float*) * (size_t)numrows);
        if(!rows) goto DONE;
        memcpy(flat, dm, sizeof(float) * (size_t)numrows * padded);
        for(int i = 0; i < numrows; i++) rows[i] = flat + (size_t)i * padded;
        for(int k = 0; k < tries; k++){
                struct kmeans_result* res = NULL;
                if(split2(rows, samples, num_anchors, num_samples, k * step, &res) != OK || !res) goto DONE;
                score[k] = res->score;
                nlr[2 * k] = res->nl; nlr[2 * k + 1] = res->nr;
                memcpy(lists + (size_t)(2 * k) * num_samples, res->sl, sizeof(int) * (size_t)res->nl);
                memcpy(lists + (size_t)(2 * k + 1) * num_samples, res->sr, sizeof(int) * (size_t)res->nr);
                free_kmeans_results(res);
        }
        rc = 0;
DONE:
        free(rows);
        free(flat);
        return rc;
}
