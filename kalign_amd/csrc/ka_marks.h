// ka_marks.h -- which edges a KALIGN_REFINE_CONFIDENT pass refines: the trees of a job's task list and the median rule of
// compute_confidence_threshold (aln_refine.c:674-712) per tree.  Host only, no context and no device handle: ka_api.cpp's
// refinement entry and the tests' seam ka_debug_refine_marks (include/kalign_amd.h) share it.
#pragma once
#include <string>
#include <vector>

struct KaMarks {
        std::vector<int> tree_of;      // [n_tasks] the tree a task belongs to; trees numbered by ascending index of their root task
        std::vector<float> thr;        // [n_trees] the threshold every tree's tasks are compared with
        std::vector<char> mark;        // [n_tasks] conf[t] <= thr[tree_of[t]]
        int n_trees = 0;
};

// tasks_abc: the job's task list, children before parents, as ka_tree_upload takes it (a forest: any number of roots, their
// trees' tasks in any interleaving).  conf[n_tasks]: a confidence per task; NULL: only the trees (thr 0, nothing marked).
// pooled: ONE median over all tasks, whatever tree they are of, is every tree's threshold.  Returns 0, or 1 with the cause in err.
__attribute__((visibility("hidden"))) int ka_refine_marks(int numseq, int n_tasks, const int* tasks_abc, const float* conf, bool pooled,
                                                          KaMarks& out, std::string& err);
