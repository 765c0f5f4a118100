// ka_marks.cpp -- the marks of a KALIGN_REFINE_CONFIDENT pass (ka_marks.h), and the seam that hands them to the tests.
// Host only: nothing here includes a device header, so the unit compiles and runs on its own (a main that defines fail()).
#include "ka_marks.h"

#include <algorithm>

#include "kalign_amd.h"

// the thread's error text (ka_last_error): defined in ka_api.cpp
__attribute__((visibility("hidden"))) int fail(const std::string& m);

// compute_confidence_threshold (aln_refine.c:674-712): the median of the sorted values, in fp32
static float median_of(std::vector<float>& v)
{
        std::sort(v.begin(), v.end());
        const size_t n = v.size();
        return (n % 2 == 0) ? (v[n / 2 - 1] + v[n / 2]) / 2.0F : v[n / 2];
}

int ka_refine_marks(int numseq, int n_tasks, const int* abc, const float* conf, bool pooled, KaMarks& out, std::string& err)
{
        if (numseq < 2 || n_tasks < 1 || n_tasks > numseq - 1 || !abc) { err = "need numseq >= 2 and 1 <= n_tasks <= numseq-1"; return 1; }
        const int nprof = 2 * numseq - 1;
        // ---- one forward pass over the list: who makes a node, who consumes it (the checks are prepare_tasks', ka_plan.cpp) ----
        std::vector<char> made(nprof, 0);                // 1 made, 2 made and consumed
        std::vector<int> maker(nprof, -1), parent(n_tasks, -1);
        for (int i = 0; i < numseq; i++) made[i] = 1;
        for (int t = 0; t < n_tasks; t++) {
                const int a = abc[3 * (size_t)t], b = abc[3 * (size_t)t + 1], c = abc[3 * (size_t)t + 2];
                if (a < 0 || b < 0 || c < numseq || a >= nprof || b >= nprof || c >= nprof || !made[a] || !made[b] || made[c]) {
                        err = "task " + std::to_string(t) + ": the task list is not in TASK_ORDER_TREE order (children before parents)";
                        return 1;
                }
                if (a == b || made[a] == 2 || made[b] == 2) {
                        err = "task " + std::to_string(t) + ": the task list is not in TASK_ORDER_TREE order (a node is consumed twice)";
                        return 1;
                }
                made[a] = 2; made[b] = 2; made[c] = 1;
                maker[c] = t;
                if (a >= numseq) parent[maker[a]] = t;
                if (b >= numseq) parent[maker[b]] = t;
        }
        // ---- a root is a task nobody consumes; trees by ascending root; a task's tree is its parent's (parents come later) ----
        out.tree_of.assign(n_tasks, -1);
        out.n_trees = 0;
        for (int t = 0; t < n_tasks; t++) if (parent[t] < 0) out.tree_of[t] = out.n_trees++;
        for (int t = n_tasks - 1; t >= 0; t--) if (parent[t] >= 0) out.tree_of[t] = out.tree_of[parent[t]];
        out.thr.assign(out.n_trees, 0.0f);
        out.mark.assign(n_tasks, 0);
        if (!conf) return 0;
        // ---- the median rule, per tree or pooled ----
        if (pooled) {
                std::vector<float> v(conf, conf + n_tasks);
                out.thr.assign(out.n_trees, median_of(v));
        } else {
                std::vector<std::vector<float>> v(out.n_trees);
                for (int t = 0; t < n_tasks; t++) v[out.tree_of[t]].push_back(conf[t]);
                for (int k = 0; k < out.n_trees; k++) out.thr[k] = median_of(v[k]);
        }
        for (int t = 0; t < n_tasks; t++) out.mark[t] = conf[t] <= out.thr[out.tree_of[t]] ? 1 : 0;
        return 0;
}

extern "C" int ka_debug_refine_marks(int numseq, int n_tasks, const int* tasks_abc, const float* conf, int pooled,
                                     int* tree_of_out, float* thr_out, int* marks_out, int* n_trees_out)
{
        if (!tasks_abc || !conf || !tree_of_out || !thr_out || !marks_out || !n_trees_out) return fail("ka_debug_refine_marks: null argument");
        KaMarks m;
        std::string err;
        if (ka_refine_marks(numseq, n_tasks, tasks_abc, conf, pooled != 0, m, err)) return fail("ka_debug_refine_marks: " + err);
        for (int t = 0; t < n_tasks; t++) { tree_of_out[t] = m.tree_of[t]; marks_out[t] = m.mark[t]; }
        for (int k = 0; k < m.n_trees; k++) thr_out[k] = m.thr[k];
        *n_trees_out = m.n_trees;
        return KA_OK;
}
