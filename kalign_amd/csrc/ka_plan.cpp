// ka_plan.cpp -- the launch planner of the task tree (round 5: out of ka_api.cpp): which guide-tree levels run as leaf launches, which as
// ONE queued launch, from where the rest of the tree is ONE chained launch; the workgroup table of every launch; the spare workgroups of
// the chained launch by a greedy pass over a simulated schedule (DESIGN.md sections 4, 4d, 4h).  Replaces the task order of
// create_msa_tree / recursive_aln (lib/src/aln_run.c:43-124) -- the reference walks the tree with OpenMP tasks.
// The planner proper (prepare_tasks, build_blocks, plan_launches and its steps) works on a KaPlan (ka_plan.h) and needs no GPU; the
// context comes in with ka_tree_upload and upload_plan, and ka_debug_plan / ka_debug_ctx_plan hand a plan out for tests and tools.
#include "ka_ctx.h"

// mean seq_distance over both clusters in sip order (aln_run.c:126-203)
static float mean_distance(const float* dist, const std::vector<int>& ma, const std::vector<int>& mb, int numseq, int* count)
{
        float sum = 0.0f;
        int n = 0;
        for (int x : ma) if (x < numseq) { sum += dist[x]; n++; }
        for (int x : mb) if (x < numseq) { sum += dist[x]; n++; }
        *count = n;
        return n ? sum / (float)n : 0.0f;
}

// Workgroup table of one launch: near the top of the tree there are fewer tasks than CUs, so a task
// gets a cluster of up to max_cluster workgroups (the kernel decides from the actual operand
// lengths how many of them it uses).  Workgroups of one cluster are spaced 8 blocks apart:
// block b runs on XCD b % 8 (observed, not contractual -- used for L2 locality only).
void build_blocks(const KaPlan* c, const std::vector<int>& L, std::vector<int2>& tbl, int* lean_out)
{
        const int nt = (int)L.size();
        int lean = 1;                                    // launch kind: 0 = 8 waves, 1 = lean, 2 = half
        for (int t : L) if (c->descs[t].nsip_a != 1 || c->descs[t].nsip_b != 1) lean = 0;
        if (c->env.no_lean) lean = 0;
        if (!lean && nt > c->n_cus && !c->env.no_half) lean = 2;   // more tasks than CUs: two 4-wave workgroups per CU
        int G = 1;
        while (lean == 0 && G * 2 <= c->max_cluster && nt * G * 2 <= c->n_cus) G *= 2;
        const int groups = (nt + 7) / 8;
        tbl.assign((size_t)groups * 8 * G, make_int2(-1, 0));
        for (int j = 0; j < nt; j++)
                for (int m = 0; m < G; m++)
                        tbl[(size_t)(j % 8) + 8 * ((size_t)m + (size_t)G * (j / 8))] = make_int2(L[j], m | (G << 8));
        *lean_out = lean;
}

// ---- the launch planner: plan_launches at the end of this part is the list of its steps ----
// The tasks a plan covers: all of them, or the subset of ka_tree_plan_tasks (a rank's subtrees of a sharded tree: closed under
// descendants).  A task outside the plan is neither a parent nor a producer in it.
static inline bool act(const KaPlan* p, int t) { return p->plan_active.empty() || p->plan_active[t] != 0; }
// a task of the chained launch: a task of the plan at or above the chain's first level
static inline bool in_chain(const KaPlan* p, int t) { return t >= 0 && act(p, t) && p->task_level[t] >= p->chain_level; }
static bool all_seq_seq(const KaPlan* p, const std::vector<int>& L)
{
        return std::all_of(L.begin(), L.end(), [&](int t) { return p->descs[t].nsip_a == 1 && p->descs[t].nsip_b == 1; });
}

// What the steps of one plan hand each other (local to a plan_launches call).
struct PlanWork {
        std::vector<int> task_of;                    // node -> the task that makes it (-1: a sequence)
        // Profile lengths are only known on the device; the estimate per node, in two models.  len_sqrt: the longest member sequence
        // times (1 + 0.1 sqrt(members)) -- the growth of the DSSim sets with their indel-rich tails (13151 columns for 4096 x 2000 nt,
        // 2965 for 4096 x 400 aa), harmless where alignments stay shorter.  len_11: 1.1 x the longer child, compounding (round 3).
        std::vector<double> len_sqrt, len_11;
        // ... and per task, in either model, the way to the root: estimated wavefront steps (2 max + min of the operands' lengths) of the
        // task and of everything above it in the plan.
        std::vector<double> way_sqrt, way_11;
        int L0 = 0;                                  // the first level that is not all seq-seq (at most chain_level; 0 without a chain)
        std::vector<int> order, extra;               // the chain's entries in layout order; spare workgroups of each, beyond G0
        int m = 0, G0 = 1, spare = 0;                // entries per XCD column; workgroups every entry starts with; CUs still free
};

// parents (of the plan), roots (of the tree), trees
static void link_tasks(KaPlan* p, PlanWork& w)
{
        const int numseq = p->numseq, n_tasks = p->n_tasks;
        const int* abc = p->abc.data();
        w.task_of.assign(2 * numseq - 1, -1);
        for (int t = 0; t < n_tasks; t++) w.task_of[abc[3 * t + 2]] = t;
        for (int t = 0; t < n_tasks; t++) { p->descs[t].parent = -1; p->descs[t].chain_need = 0; p->descs[t].is_root = 1; p->descs[t].qa = -1; p->descs[t].qb = -1; }
        for (int t = 0; t < n_tasks; t++)
                for (int k = 0; k < 2; k++) {
                        const int ch = abc[3 * t + k];
                        if (ch < numseq) continue;
                        // (is_root is a property of the tree: the root's task builds no profile.  parent is one of the plan.)
                        p->descs[w.task_of[ch]].is_root = 0;
                        if (act(p, t) && act(p, w.task_of[ch])) p->descs[w.task_of[ch]].parent = t;
                }
        p->n_trees = numseq - n_tasks;
}

// The one estimator: lengths per node, ways to the root per task, both models, once per plan (the queue-order and spare
// steps read them), and with the lengths the tasks' wait_mult.  Every sum keeps its operand order -- the steps sort on these
// doubles, and the plans are pinned bit for bit (tests/test_plan_host.py).
static void estimate(KaPlan* p, PlanWork& w)
{
        const int numseq = p->numseq, n_tasks = p->n_tasks;
        const int* abc = p->abc.data();
        std::vector<double> lmax(2 * numseq - 1, 0.0), nmem(2 * numseq - 1, 1.0), cells(2 * numseq - 1, 0.0);
        w.len_sqrt.assign(2 * numseq - 1, 0.0); w.len_11.assign(2 * numseq - 1, 0.0);
        for (int i = 0; i < numseq; i++) { lmax[i] = p->lens[i]; w.len_sqrt[i] = p->lens[i]; w.len_11[i] = p->lens[i]; }
        for (int t = 0; t < n_tasks; t++) {
                const int a = abc[3 * t], b = abc[3 * t + 1], cc = abc[3 * t + 2];
                lmax[cc] = std::max(lmax[a], lmax[b]); nmem[cc] = nmem[a] + nmem[b];
                w.len_sqrt[cc] = lmax[cc] * (1.0 + 0.1 * std::sqrt(nmem[cc]));
                w.len_11[cc] = 1.1 * std::max(w.len_11[a], w.len_11[b]);
                // join watchdog of the chained launch: ~2 s per 4e9 estimated DP cells below the task (a healthy sibling subtree of a
                // huge job may legitimately take longer than the base bound); always by the compounding model
                cells[cc] = cells[a] + cells[b] + w.len_11[a] * w.len_11[b];
                p->descs[t].wait_mult = 1 + (int)std::min(63.0, cells[cc] / 4e9);
                // (descs[t].refine -- the edges a KALIGN_REFINE_CONFIDENT pass refines -- is not part of the plan: it is
                // set by ka_tree_refine and must survive the re-plan of a watchdog fallback, ka_tree_sync)
        }
        // (the steps once guarded the parent's term differently -- `active and has a parent` in three, `has a parent` in the spare pass.
        // One guard serves both: link_tasks gives a parent to tasks of the plan only, so a task outside it has none.)
        w.way_sqrt.assign(n_tasks, 0.0); w.way_11.assign(n_tasks, 0.0);
        for (int t = n_tasks - 1; t >= 0; t--) {                      // parents come after their children in the task list
                const int a = abc[3 * t], b = abc[3 * t + 1], up = p->descs[t].parent;
                w.way_sqrt[t] = 2.0 * std::max(w.len_sqrt[a], w.len_sqrt[b]) + std::min(w.len_sqrt[a], w.len_sqrt[b]) + (up >= 0 ? w.way_sqrt[up] : 0.0);
                w.way_11[t] = 2.0 * std::max(w.len_11[a], w.len_11[b]) + std::min(w.len_11[a], w.len_11[b]) + (up >= 0 ? w.way_11[up] : 0.0);
        }
}

// The level from which the rest of the tree runs as ONE chained launch: the first non-leaf level with at most one task per CU (all
// its workgroups resident at once; levels only get narrower above it).  KA_NO_CHAIN=1 keeps one launch per level.  And w.L0, the
// first level below it that is not all seq-seq: where a queued launch would start.
static void place_chain(KaPlan* p, PlanWork& w)
{
        p->chain_level = -1;
        if (p->env.no_chain || p->shared_gpu) return;
        // (one tree: the chain starts where a level has at most 200 tasks -- the ~50 workgroups that leaves free go to the
        // entries under the critical path, and since the chain overlaps the queue (round 5) a later start costs little:
        // 4096 x 400 aa 14.70 -> 14.61 ms, default mode 21.4 -> 20.6, 4096 x 2000 nt 71.8 -> 70.2, 1024 x 2000 nt 33.3 -> 31.9;
        // a forest keeps every CU it can get: four 4096 x 2000 nt trees 183 -> 191 with 200; profiles/r05_chain_start.log)
        int chain_tasks = (p->n_trees <= 1) ? std::min(p->n_cus - 8, 200) : p->n_cus - 8;
        if (p->env.chain_tasks > 0) chain_tasks = std::min(chain_tasks, p->env.chain_tasks);   // experiments
        for (int L = 0; L + 1 < (int)p->plan_levels.size(); L++)
                if (!all_seq_seq(p, p->plan_levels[L]) && (int)p->plan_levels[L].size() <= chain_tasks) { p->chain_level = L; break; }   // one workgroup per CU, all resident
        while (w.L0 < p->chain_level && all_seq_seq(p, p->plan_levels[w.L0])) w.L0++;    // the leading seq-seq levels (lean kernel) end here
}

// The queued launch: every level between the seq-seq leaves and the chained launch (each holds more tasks than the GPU has
// workgroup slots) as ONE launch of the half kernel; see ka_task_queue_entry.  KA_NO_QUEUE=1 keeps one launch per level.
// Overlapping launches (KA_OVERLAP; whole-tree plans only): the chained launch goes out beside the queued one, and its tasks wait
// for the done flags of what the QUEUE makes for them (set_queue_deps).
static void place_queue(KaPlan* p, const PlanWork& w)
{
        p->queue_first = -1;
        p->overlap_plan = 0;
        if (p->chain_level < 1 || p->env.no_queue || p->env.no_half) return;
        if (p->chain_level - w.L0 < 2) return;                                  // one level alone gains nothing
        if ((int)p->plan_levels[w.L0].size() <= p->n_cus) return;               // (the queue's first level must fill the GPU; later ones need not)
        p->queue_first = w.L0;
        p->overlap_plan = (p->env.overlap > 0 && p->plan_active.empty() && !p->env.no_lean && !p->shared_gpu) ? p->env.overlap : 0;
}

// join counts of the chained launch: the children of a task that run inside it
static void set_chain_need(KaPlan* p, const PlanWork& w)
{
        if (p->chain_level < 0) return;
        for (int t = 0; t < p->n_tasks; t++) {
                if (!in_chain(p, t)) continue;
                int need = 0;
                for (int k = 0; k < 2; k++) {
                        const int ch = p->abc[3 * t + k];
                        if (ch >= p->numseq && in_chain(p, w.task_of[ch])) need++;
                }
                p->descs[t].chain_need = need;
        }
        // tests: make the last join wait for a workgroup that never comes (a residency failure as seen
        // from the device) -- the bounded wait must report it and ka_tree_sync must re-plan and re-run
        if (p->test_hooks & KA_DEBUG_STARVE_ROOT_JOIN) p->descs[p->n_tasks - 1].chain_need += 1;
}

// qa / qb: the producers of a task's operands in the queued launch -- for the queue's own tasks, and in an overlapping plan for the
// chain's tasks too: its operands' producers in the queued launch (inside the chain the join points order things as before).
static void set_queue_deps(KaPlan* p, const PlanWork& w)
{
        if (p->queue_first < 0) return;
        const int lo = p->queue_first;
        for (int t = 0; t < p->n_tasks; t++) {
                if (p->task_level[t] < lo || !act(p, t)) continue;
                // (a task of the chained launch: only what OTHER launches make -- inside the chain the join points order things)
                const bool chained = in_chain(p, t);
                if (chained && !p->overlap_plan) continue;
                auto dep = [&](int node) -> int {
                        if (node < p->numseq || !act(p, w.task_of[node])) return -1;
                        const int lv = p->task_level[w.task_of[node]];
                        if (lv < lo || (chained && in_chain(p, w.task_of[node]))) return -1;
                        return w.task_of[node];
                };
                p->descs[t].qa = dep(p->abc[3 * t]);
                p->descs[t].qb = dep(p->abc[3 * t + 1]);
        }
}

// Workgroups one task may use: 16, or 32 for jobs whose top tasks are big enough to be work-bound at 16 (round 4: a
// 9000 x 9700 task of C3 takes 5.8 ms on 16 workgroups, of which ~1.6 ms are the wavefront's dependent steps) -- by the
// estimated root (longest sequence x (1 + 0.1 sqrt(sequences)), squared): >= 6e7 cells.  Measured, limit 16 -> 32
// (profiles/r04_max_cluster.log): C3 81.9 -> 74.8 ms, 1024 x 2000 nt 34.9 -> 33.0, 512 x 3000 nt 43.6 -> 41.9; 16384 x 500 aa
// and 2048 x 1000 aa unchanged; 4096 x 400 aa and 8192 x 300 aa 1-2 % slower (surplus members waiting at the joins).
static void set_cluster_limit(KaPlan* p)
{
        double lmax = 0.0;
        for (int i = 0; i < p->numseq; i++) lmax = std::max(lmax, (double)p->lens[i]);
        const double root = lmax * (1.0 + 0.1 * std::sqrt((double)p->numseq));
        // (... and for big jobs with a consistency table: the votes of their top tasks share by member ranges from 20 workgroups on)
        const bool big_cons = p->cons_K > 0 && p->numseq >= 2048;
        p->max_cluster = p->env.max_cluster > 0 ? std::min(32, p->env.max_cluster) : ((root * root >= 6e7 || big_cons) ? 32 : 16);
        if (p->shared_gpu) p->max_cluster = 1;
}

// workgroup tables, one per dependency level (build_blocks)
static void build_level_tables(KaPlan* p)
{
        p->blocks_flat.clear(); p->blocks_off.assign(1, 0); p->level_lean.clear();
        for (auto& L : p->plan_levels) {
                std::vector<int2> tbl;
                int lean = 0;
                build_blocks(p, L, tbl, &lean);
                p->level_lean.push_back(lean);
                p->blocks_flat.insert(p->blocks_flat.end(), tbl.begin(), tbl.end());
                p->blocks_off.push_back((int)p->blocks_flat.size());
        }
}

// The queue's task list.  Within a level the tasks with the longest way to the root go first (estimated wavefront steps of the task
// and of everything above it, as for the chain's spare workgroups below): what the chained launch waits for longest -- the
// spine of a caterpillar tree -- then leaves the queue early instead of wherever the task list put it.  KA_QORDER=0: list order.
static void order_queue(KaPlan* p, const PlanWork& w)
{
        p->queue_off = (int)p->blocks_flat.size(); p->queue_n = 0;
        if (p->queue_first < 0) return;
        const bool by_way = p->env.qorder;
        auto longer_way = [&](int x, int y) { return by_way && w.way_sqrt[x] > w.way_sqrt[y]; };
        for (int L = p->queue_first; L < p->chain_level; L++) {
                std::vector<int> run(p->plan_levels[L]);
                std::stable_sort(run.begin(), run.end(), longer_way);
                for (int t : run) { p->blocks_flat.push_back(make_int2(t, 1 << 8)); p->queue_n++; }
        }
}

// Every task of the chain's first level starts on a single workgroup; clusters form on the way up.
// Entries are laid out in depth-first order of the upper tree, one contiguous run per XCD
// (block b runs on XCD b % 8 -- observed, not contractual): subtrees that merge early share an
// L2, only the top three levels cross XCDs.
static void enter_chain(const KaPlan* p, PlanWork& w)
{
        std::vector<int> stack;
        for (int t = p->n_tasks - 1; t >= 0; t--) if (act(p, t) && p->descs[t].parent < 0 && p->task_level[t] >= p->chain_level) stack.push_back(t);   // every root above the cut
        while (!stack.empty()) {
                const int t = stack.back(); stack.pop_back();
                // an entry of the chain: no child of it runs inside the launch (the chain's first level; in a plan over a subset also
                // a task whose children were all run before)
                if (p->descs[t].chain_need == 0) { w.order.push_back(t); continue; }
                for (int k = 1; k >= 0; k--) {
                        const int ch = p->abc[3 * t + k];
                        if (ch >= p->numseq && in_chain(p, w.task_of[ch])) stack.push_back(w.task_of[ch]);
                }
        }
        w.m = ((int)w.order.size() + 7) / 8;
        w.extra.assign(w.order.size(), 0);
        // A narrow upper tree (the chain-like UPGMA trees of a realignment pass) never merges clusters: its
        // tasks would all run on the one workgroup they started with.  Start with as many workgroups per
        // task as a separate launch of this level would get (build_blocks); members of one cluster sit in
        // one column = one XCD.
        w.G0 = 1;
        while (w.G0 * 2 <= p->max_cluster && 8 * w.m * w.G0 * 2 <= p->n_cus) w.G0 *= 2;
        if (p->env.chain_g1) w.G0 = 1;
        w.spare = (p->n_cus - 8 * w.m * w.G0) / 8 * 8;
}

// Round 4: first a GREEDY pass on a simulated schedule.  The ranking below only knows how LONG an entry's way
// to the root is, not how it will be staffed: a caterpillar spine that absorbs siblings finished by earlier
// launches stays on the one workgroup of its entry through level after level of 2400 x 2300 tasks (C3: six
// of them at 3.8 ms, a third of the launch, next to ~200 idle CUs) while a spine fed by subtrees of THIS
// launch collects their workgroups at every join.  Model: a task on G workgroups takes
// a * (2 max + min) + b * la * lb / G (fitted on C3's and the headline's task times: the first term the
// wavefront's dependent steps, the second the cells shared by the cluster; b / a = 0.02 from the fit, 0.01 in use), a parent has the
// workgroups of its children in this launch (up to the limit) and starts when the later one ends.  One spare
// workgroup at a time goes to the entry under the simulated critical path, until it stops paying; what is
// left goes out by the ranking.  KA_CRIT_GREEDY=0: the ranking alone (round 3).
static void spare_by_simulation(const KaPlan* p, PlanWork& w, const std::vector<double>& len)
{
        const int numseq = p->numseq, n_tasks = p->n_tasks;
        const int* abc = p->abc.data();
        std::vector<int>& extra = w.extra;
        std::vector<int> entry_of(n_tasks, -1);
        for (size_t r = 0; r < w.order.size(); r++) entry_of[w.order[r]] = (int)r;
        std::vector<double> fin(n_tasks, 0.0);
        std::vector<int> Gt(n_tasks, 0), crit_child(n_tasks, -1);
        const double ba = 0.01;                              // (b / a of the model: from a sweep over five job shapes, profiles/r04_crit_ba.log)
        auto simulate = [&]() -> int {
                int last = -1;
                for (int t = 0; t < n_tasks; t++) {                  // children come before their parents
                        if (!in_chain(p, t)) continue;
                        double start = 0.0; int cc = -1, G = 0;
                        if (entry_of[t] >= 0) G = w.G0 + extra[entry_of[t]];
                        else {
                                for (int k = 0; k < 2; k++) {
                                        const int ch = abc[3 * t + k];
                                        const int tc = ch >= numseq ? w.task_of[ch] : -1;
                                        if (!in_chain(p, tc)) continue;
                                        G += Gt[tc];
                                        if (fin[tc] >= start) { start = fin[tc]; cc = tc; }
                                }
                                G = std::max(1, std::min(G, p->max_cluster));
                        }
                        const double la = len[abc[3 * t]], lb = len[abc[3 * t + 1]];
                        fin[t] = start + 2.0 * std::max(la, lb) + std::min(la, lb) + ba * la * lb / G;
                        Gt[t] = G; crit_child[t] = cc;
                        if (last < 0 || fin[t] > fin[last]) last = t;
                }
                return last;                                       // the task that ends last (a root)
        };
        // (several paths can be critical at once: a workgroup that shortens ONE of them leaves the end where it was.
        // Keep going -- the next round takes the next path -- and fall back to the best state seen when a
        // stretch of eight additions has not moved the end.)
        int given = 0, since_best = 0;
        std::vector<int> best_extra = extra;
        int best_spare = w.spare;
        double best_end = -1.0;
        { const int t = simulate(); if (t >= 0) best_end = fin[t]; }
        while (w.spare > 0 && best_end > 0.0 && since_best < 8) {
                int t = simulate();
                if (t < 0) break;
                while (crit_child[t] >= 0) t = crit_child[t];        // down the critical path to its entry
                const int r = entry_of[t];
                if (r < 0 || w.G0 + extra[r] >= p->max_cluster) break;
                extra[r] += 1; w.spare -= 1;
                const int t2 = simulate();
                if (fin[t2] < best_end * (1.0 - 1e-4)) { best_end = fin[t2]; best_extra = extra; best_spare = w.spare; since_best = 0; }
                else since_best += 1;
        }
        extra = best_extra; w.spare = best_spare;
        for (size_t r = 0; r < w.order.size(); r++) given += extra[r];
        if (p->env.plan_verbose) {
                const int t = simulate();
                fprintf(stderr, "chain plan: greedy pass gave %d workgroups, %d left for the ranking; simulated end %.0f\n", given, w.spare, t >= 0 ? fin[t] : 0.0);
                for (size_t r = 0; r < w.order.size(); r++) if (extra[r] > 0)
                        fprintf(stderr, "  entry task %d (node %d) level %d: +%d\n", w.order[r], abc[3 * w.order[r] + 2], p->task_level[w.order[r]], extra[r]);
        }
}

// ... then the ranking: what is left goes to the entries in the order of their way to the root
static void spare_by_ranking(const KaPlan* p, PlanWork& w, const std::vector<double>& len, const std::vector<double>& up)
{
        const int* abc = p->abc.data();
        std::vector<int> by_up(w.order.size());
        for (size_t r = 0; r < w.order.size(); r++) by_up[r] = (int)r;
        std::stable_sort(by_up.begin(), by_up.end(), [&](int x, int y) { return up[w.order[x]] > up[w.order[y]]; });
        int top_g = 4;
        if (p->env.crit_top > 0) top_g = std::min(p->max_cluster, p->env.crit_top);   // experiments
        for (size_t i = 0; i < by_up.size() && w.spare > 0; i++) {
                // (never beyond the cluster limit: surplus workgroups would only spin at a join and leave)
                const int want = std::min(w.spare, std::max(0, std::min(p->max_cluster, i == 0 ? top_g : 2 * w.G0) - w.G0 - w.extra[by_up[i]]));
                w.extra[by_up[i]] += want; w.spare -= want;
        }
        if (p->env.plan_verbose) {
                fprintf(stderr, "chain plan: level %d, %zu entries, G0 %d, spare after extras %d, top_g %d\n", p->chain_level, w.order.size(), w.G0, w.spare, top_g);
                for (size_t i = 0; i < by_up.size() && i < 12; i++) {
                        const int t = w.order[by_up[i]];
                        fprintf(stderr, "  rank %zu: task %d (node %d) level %d lens %.0f x %.0f up %.0f extra %d\n", i, t, abc[3 * t + 2], p->task_level[t],
                                len[abc[3 * t]], len[abc[3 * t + 1]], up[t], w.extra[by_up[i]]);
                }
        }
}

// The CUs the entries leave idle go to the entries whose way to the root is the longest (estimated wavefront steps
// of the tasks above them): clusters only grow where subtrees of the SAME launch meet, and the critical path
// of a k-means tree is a caterpillar that absorbs small subtrees finished by earlier launches -- its tasks
// would run on the one workgroup their entry started with while most of the GPU waits at join points.  A
// cluster keeps its workgroups all the way up (surplus members climb with it), so a workgroup given to an
// entry serves every task on that entry's path.  Extra members sit behind the regular table, in the
// entry's XCD column.
static void give_spare_workgroups(const KaPlan* p, PlanWork& w)
{
        if (p->env.no_crit || w.spare <= 0 || w.order.empty()) return;
        // (the greedy pass and the ranking behind it read the square-root model; KA_CRIT_GREEDY=0, the ranking alone, the compounding one)
        const std::vector<double>& len = p->env.crit_greedy ? w.len_sqrt : w.len_11;
        const std::vector<double>& up = p->env.crit_greedy ? w.way_sqrt : w.way_11;
        if (p->env.crit_greedy) spare_by_simulation(p, w, len);
        spare_by_ranking(p, w, len, up);
}

// the chained launch's block table: 8 XCD columns of m entries with G0 workgroups each, the spare workgroups behind them
static void lay_out_chain(KaPlan* p, PlanWork& w)
{
        const int m = w.m, G0 = w.G0;
        int n_extra = 0;
        std::vector<int> col_need(8, 0);
        for (size_t r = 0; r < w.order.size(); r++) { n_extra += w.extra[r]; col_need[r / m] += w.extra[r]; }
        int extra_rows = *std::max_element(col_need.begin(), col_need.end());
        const bool by_column = 8 * m * G0 + 8 * extra_rows <= p->n_cus;       // else: packed densely, any XCD
        if (!by_column) extra_rows = (n_extra + 7) / 8;
        p->chain_blocks.assign((size_t)8 * m * G0 + (size_t)8 * extra_rows, make_int2(-1, 0));
        std::vector<int> col_fill(8, 0);
        int dense = 0;
        for (int r = 0; r < (int)w.order.size(); r++) {
                const int Gr = G0 + w.extra[r];
                for (int g = 0; g < G0; g++)
                        p->chain_blocks[((size_t)(r % m) * G0 + g) * 8 + (r / m)] = make_int2(w.order[r], g | (Gr << 8));
                for (int g = G0; g < Gr; g++) {
                        const size_t pos = (size_t)8 * m * G0 + (by_column ? (size_t)8 * col_fill[r / m]++ + (r / m) : (size_t)dense++);
                        p->chain_blocks[pos] = make_int2(w.order[r], g | (Gr << 8));
                }
        }
        p->chain_blocks_off = (int)p->blocks_flat.size();
        p->blocks_flat.insert(p->blocks_flat.end(), p->chain_blocks.begin(), p->chain_blocks.end());
}

// Launch plan of the prepared job: parents and join counts of the chained launch, workgroup tables per level.
// Depends on p->shared_gpu (no clusters, no chain), so ka_tree_sync can re-plan after a residency failure.
int plan_launches(KaPlan* p)
{
        PlanWork w;
        p->plan_levels.assign(p->levels.size(), std::vector<int>());
        for (size_t L = 0; L < p->levels.size(); L++) for (int t : p->levels[L]) if (act(p, t)) p->plan_levels[L].push_back(t);
        link_tasks(p, w);
        estimate(p, w);
        // which launches there are
        place_chain(p, w);
        place_queue(p, w);
        set_chain_need(p, w);
        set_queue_deps(p, w);
        // their workgroup tables: one per level, the queue's list, the chain's table
        set_cluster_limit(p);
        build_level_tables(p);
        order_queue(p, w);
        if (p->chain_level >= 0) {
                enter_chain(p, w);
                give_spare_workgroups(p, w);
                lay_out_chain(p, w);
        }
        return KA_OK;
}

// Host-side task preparation of an upload: the order checks of the task list, nsip, sip order, gap_scale / subm_offset, levels.
// Fills the job part of the KaPlan; needs no GPU (ka_tree_upload and ka_debug_plan share it).
int prepare_tasks(KaPlan* c, int numseq, const int* lens, const float* seq_distances, int n_tasks, const int* abc, const float* scal)
{
        const int nprof = 2 * numseq - 1;
        c->numseq = numseq; c->n_tasks = n_tasks;
        c->lens.assign(lens, lens + numseq);
        c->abc.assign(abc, abc + 3 * n_tasks);
        c->sip_flat.clear(); c->sip_off.assign(nprof, 0);
        for (int i = 0; i < numseq; i++) { c->sip_off[i] = (long long)c->sip_flat.size(); c->sip_flat.push_back(i); }

        // ---- host-side task preparation: nsip, sip order, gap_scale / subm_offset, levels ----
        std::vector<int> nsip(nprof, 0), level(nprof, 0);
        std::vector<std::vector<int>> sip(nprof);
        std::vector<char> made(nprof, 0);
        for (int i = 0; i < numseq; i++) { nsip[i] = 1; sip[i] = {i}; made[i] = 1; }
        c->descs.assign(n_tasks, KaTaskDesc());
        const float gpo0 = scal[0], gpe0 = scal[1], tgpe0 = scal[2], dist_scale = scal[3], vsm_amax = scal[4];
        int max_level = 0;
        for (int t = 0; t < n_tasks; t++) {
                const int a = abc[3 * t], b = abc[3 * t + 1], cc = abc[3 * t + 2];
                if (a < 0 || b < 0 || cc < numseq || a >= nprof || b >= nprof || cc >= nprof || !made[a] || !made[b] || made[cc])
                        return fail("task list is not in TASK_ORDER_TREE order (children before parents)");
                // a node is the operand of at most one task, and never both operands of it (its member list is
                // handed to the parent below)
                if (a == b || made[a] == 2 || made[b] == 2)
                        return fail("task list is not in TASK_ORDER_TREE order (a node is consumed twice)");
                made[a] = 2; made[b] = 2;
                KaTaskDesc& d = c->descs[t];
                float gap_scale = 1.0f, soff = 0.0f;
                int cnt = 0;
                if (dist_scale > 0.0f && seq_distances) {
                        const float avg = mean_distance(seq_distances, sip[a], sip[b], numseq, &cnt);
                        if (cnt) {
                                gap_scale = 1.0f - dist_scale * avg;
                                if (gap_scale < 0.3f) gap_scale = 0.3f;
                                if (gap_scale > 1.0f) gap_scale = 1.0f;
                        }
                }
                if (vsm_amax > 0.0f && seq_distances) {
                        const float avg = mean_distance(seq_distances, sip[a], sip[b], numseq, &cnt);
                        if (cnt) {
                                soff = vsm_amax - avg;
                                if (soff < 0.0f) soff = 0.0f;
                        }
                }
                d.a = a; d.b = b; d.c = cc;
                d.nsip_a = nsip[a]; d.nsip_b = nsip[b];
                d.is_root = 0;                                   // set below: tasks nobody consumes
                d.gpo = gpo0; d.gpe = gpe0; d.tgpe = tgpe0;
                if (gap_scale < 1.0f || soff > 0.0f) { d.gpo *= gap_scale; d.gpe *= gap_scale; d.tgpe *= gap_scale; }
                else soff = 0.0f;
                d.soff = soff; d.gap_scale = gap_scale; d.parent = -1; d.chain_need = 0;
                nsip[cc] = nsip[a] + nsip[b];
                sip[cc].reserve(nsip[cc]);
                for (int j = nsip[a]; j--;) sip[cc].push_back(sip[a][j]);        // aln_run.c:428-436
                for (int j = nsip[b]; j--;) sip[cc].push_back(sip[b][j]);
                c->sip_off[cc] = (long long)c->sip_flat.size();
                c->sip_flat.insert(c->sip_flat.end(), sip[cc].begin(), sip[cc].end());
                std::vector<int>().swap(sip[a]);
                std::vector<int>().swap(sip[b]);
                made[cc] = 1;
                level[cc] = 1 + std::max(level[a], level[b]);
                max_level = std::max(max_level, level[cc]);
        }
        c->levels.assign(max_level, std::vector<int>());
        for (int t = 0; t < n_tasks; t++) c->levels[level[abc[3 * t + 2]] - 1].push_back(t);

        c->task_level.assign(n_tasks, 0);
        for (int t = 0; t < n_tasks; t++) c->task_level[t] = level[abc[3 * t + 2]] - 1;
        return KA_OK;
}

extern "C" int ka_tree_upload(ka_ctx* c, int numseq, const uint8_t* codes, const int* off, const int* lens,
                              const float* seq_distances, int n_tasks, const int* abc,
                              const float* subm, const float* scal, int flags)
{
        if (!c) return fail("null ctx");
        // n_tasks == numseq-1: one guide tree.  Fewer tasks: a FOREST -- several independent alignments (a batch of
        // families, ensemble members) scheduled together; every task with no consumer is the root of its tree.
        if (numseq < 2 || n_tasks < 1 || n_tasks > numseq - 1) return fail("need numseq >= 2 and 1 <= n_tasks <= numseq-1");
        HIPCHK(hipSetDevice(c->device));
        const int nprof = 2 * numseq - 1;
        // kalign_run_realign aligns a second time on a new tree with the consistency table of the first pass
        // (aln_wrap.c:424-431,497-502): same sequences, new task list.  Anything else starts without a table.
        bool keep_cons = false;
        if ((flags & KA_FLAG_KEEP_CONSISTENCY) && c->have_job && c->cons_K > 0) {
                bool same = numseq == c->numseq;
                for (int i = 0; same && i < numseq; i++)
                        same = lens[i] == c->lens[i] && off[i] == c->off[i] && memcmp(codes + off[i], c->h_codes.data() + off[i], lens[i]) == 0;
                if (!same) return fail("KA_FLAG_KEEP_CONSISTENCY: the sequences differ from those the consistency table was built on");
                keep_cons = true;
        }
        c->have_job = false; c->ran = false; c->synced = false; c->state_valid = false;
        // a join watchdog of an earlier job forced the no-cluster plan: a new job gets the fast plan again (the
        // fallback is counted, ka_ctx_fallback_runs); a caller's own ka_ctx_set_shared stays
        // -- unless the fallback before it was a fast-plan job's too: then fallback_hold jobs stay on the shared plan first (ka_tree_sync)
        if (c->shared_by_fallback) {
                if (c->fallback_hold > 0) c->fallback_hold--;
                else { c->shared_gpu = false; c->shared_by_fallback = false; }
        }
        if (!keep_cons) c->cons_K = 0;           // a new job starts without a consistency table
        c->have_colof = false;
        c->rows.forget();
        c->flags = flags;
        c->off.assign(off, off + numseq);
        memcpy(c->subm, subm, sizeof(c->subm));
        memcpy(c->scal, scal, sizeof(c->scal));
        c->sum_len = 0; c->max_len = 0;
        long long codes_bytes = 0;
        int max_code = 0;
        for (int i = 0; i < numseq; i++)
                for (int j = 0; j < lens[i]; j++) max_code = std::max<int>(max_code, codes[off[i] + j]);
        if (max_code > 22) return fail("sequence code out of range (alphabet is 0..22)");
        // nucleotide alphabets use codes 0..4 (alphabet.c:206-245); proteins without B / Z / X only codes 0..19
        c->nres = (max_code < 5) ? 5 : (max_code < 20 ? 20 : 23);
        for (int i = 0; i < numseq; i++) {
                if (lens[i] < 1) return fail("zero-length sequence (the reference removes them before the dispatcher, msa_check.c:66)");
                c->sum_len += lens[i];
                c->max_len = std::max(c->max_len, lens[i]);
                codes_bytes = std::max<long long>(codes_bytes, (long long)off[i] + lens[i]);
        }

        c->h_codes.assign(codes, codes + codes_bytes);
        if (seq_distances) c->seq_dist.assign(seq_distances, seq_distances + numseq); else c->seq_dist.clear();
        if (prepare_tasks(c, numseq, lens, seq_distances, n_tasks, abc, scal)) return KA_FAIL;
        const int max_level = (int)c->levels.size();
        c->level_ids_flat.clear(); c->level_off.assign(1, 0);
        for (auto& L : c->levels) {
                c->level_ids_flat.insert(c->level_ids_flat.end(), L.begin(), L.end());
                c->level_off.push_back((int)c->level_ids_flat.size());
        }

        c->plan_active.clear();
        if (plan_launches(c)) return KA_FAIL;

        // ---- arenas ----
        c->leaf_prof_off.assign(numseq, 0);
        long long top = 0;
        for (int i = 0; i < numseq; i++) { c->leaf_prof_off[i] = top; top += (long long)(lens[i] + 2) * KA_REC; }
        c->leaf_prof_total = top;
        // merged profiles: alignment lengths are only known on the device; start with a generous
        // estimate and let ka_tree_sync grow + re-run on overflow.
        const long long worst_cols = c->sum_len * (long long)std::max(1, max_level) + 2LL * n_tasks;
        const long long est_cols = 3LL * (long long)n_tasks * (c->max_len + 2) + 1024;
        const long long cols = std::min(worst_cols, est_cols);
        c->prof_cap = std::max(c->prof_cap, top + cols * KA_REC);
        c->path_cap = std::max(c->path_cap, cols + c->sum_len + 2LL * numseq + 1024);
        long long scr = 0;
        // per level every sequence is a member of at most one task; profile lengths never exceed
        // the sum of their members' lengths
        const long long scr_level = ka_scratch_bytes_host(c->sum_len, c->sum_len, c->max_len) / 2 + (long long)numseq * (2048 + 12LL * c->max_len) + 65536;
        scr = scr_level;
        // the chained launch and the queued launch never reset the scratch counter: several levels' worth; grows on demand
        if (c->chain_level >= 0) scr = scr_level * (long long)std::min(max_level - c->chain_level, 8);
        if (c->max_cluster > 1 && !c->shared_gpu) scr *= 2;          // clusters: every member's private queues and row buffers
        if (c->queue_first >= 0) {
                // The chained launch that overlaps the queue shares its arena (no reset between the two).  Where their sum is affordable --
                // single trees: a few GB of 288 -- the arena holds both, so that a one-shot caller (the CLI, the drop-in: one alignment
                // per process) does not pay an overflow, a doubled arena and a second run of the tree on its only job.  Big
                // forests keep the larger of the two estimates (the sum asked for more than the GPU holds on a 16-tree forest) and grow on
                // demand: ka_tree_sync doubles the arena and repeats the run, once per job shape.
                const long long scr_queue = scr_level * (long long)(c->chain_level - c->queue_first);
                const long long both = scr + scr_queue;
                scr = (c->env.overlap && both <= (24LL << 30)) ? both : std::max(scr, scr_queue);
        }
        c->scratch_cap = std::max(c->scratch_cap, scr);
        c->scratch_job = scr;
        if (c->test_hooks & KA_DEBUG_SMALL_ARENAS) {
                // tests: start with arenas that are certainly too small, so that the overflow -> grow -> re-run
                // path of ka_tree_sync is exercised (also across the join points of the chained launch)
                c->prof_cap = top + 64LL * KA_REC; c->path_cap = 64; c->scratch_cap = c->scratch_job = 1 << 16;
                c->d_prof_arena.release(); c->d_path_arena.release(); c->d_scratch.release();
        }
        c->dbg_cap = (flags & KA_FLAG_DEBUG_ROWS) ? std::max<long long>(c->dbg_cap, 6LL * (cols + 2LL * n_tasks + c->sum_len)) : c->dbg_cap;

        if (c->d_codes.alloc((size_t)codes_bytes) || c->d_seq_off.alloc(numseq) || c->d_node_len.alloc(nprof) ||
            c->d_node_prof.alloc(nprof) || c->d_level_ids.alloc(c->level_ids_flat.size()) ||
            c->d_tasks.alloc(n_tasks) || c->d_recs.alloc(n_tasks) || c->d_subm.alloc(23 * 23) ||
            c->d_counters.alloc(8) || c->d_timing.alloc(8 * (size_t)n_tasks + 48 + 512) ||
            c->d_ctl.alloc((size_t)ka_ctl_bytes_host() * n_tasks) || c->d_join.alloc(n_tasks) || c->d_blocks.alloc(c->blocks_flat.size()) || c->d_error.alloc(1) || c->d_dbg_off.alloc(n_tasks) ||
            c->d_prof_arena.alloc((size_t)c->prof_cap) || c->d_path_arena.alloc((size_t)c->path_cap) ||
            c->d_scratch.alloc((size_t)c->scratch_cap) || c->d_dbg_arena.alloc((size_t)std::max<long long>(c->dbg_cap, 1)))
                return fail("hipMalloc failed");
        HIPCHK(hipMemcpyAsync(c->d_codes.p, codes, (size_t)codes_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_seq_off.p, off, sizeof(int) * numseq, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_level_ids.p, c->level_ids_flat.data(), sizeof(int) * c->level_ids_flat.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_tasks.p, c->descs.data(), sizeof(KaTaskDesc) * n_tasks, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_blocks.p, c->blocks_flat.data(), sizeof(int2) * c->blocks_flat.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_subm.p, subm, sizeof(float) * 23 * 23, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->have_job = true;
        if (((flags & KA_FLAG_DEVICE_GAPS) || keep_cons) && setup_colof(c)) { c->have_job = false; return KA_FAIL; }
        return KA_OK;
}

// (re)upload the launch plan: task descriptors (parents, join counts) and workgroup tables
int upload_plan(ka_ctx* c)
{
        if (c->d_blocks.alloc(c->blocks_flat.size())) return fail("hipMalloc failed");
        HIPCHK(hipMemcpyAsync(c->d_tasks.p, c->descs.data(), sizeof(KaTaskDesc) * c->n_tasks, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_blocks.p, c->blocks_flat.data(), sizeof(int2) * c->blocks_flat.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return KA_OK;
}


// ---- the plan, flattened for tests and tools (include/kalign_amd.h: ka_debug_plan) ----
static int export_plan(const KaPlan* p, int* scalars, int* per_task, int* blocks, int blocks_cap, int* blocks_off, int* level_lean)
{
        if (!scalars || !per_task || !blocks_off || !level_lean || (!blocks && blocks_cap > 0)) return fail("ka_debug_plan: bad arguments");
        const int n = p->n_tasks, levels = (int)p->plan_levels.size(), n_blocks = (int)p->blocks_flat.size();
        const bool chain = p->chain_level >= 0;
        const int sc[16] = { levels, n_blocks, p->max_cluster, p->n_trees, p->chain_level, p->queue_first, p->queue_off, p->queue_n, p->overlap_plan,
                             chain ? p->chain_blocks_off : 0, chain ? (int)p->chain_blocks.size() : 0, 0, 0, 0, 0, 0 };
        memcpy(scalars, sc, sizeof(sc));
        if (n_blocks > blocks_cap) return fail("ka_debug_plan: the block table needs more room (scalars[1] entries)");
        for (int t = 0; t < n; t++) {
                const KaTaskDesc& d = p->descs[t];
                const int v[6] = { d.parent, d.chain_need, d.is_root, d.wait_mult, d.qa, d.qb };
                for (int k = 0; k < 6; k++) per_task[(size_t)k * n + t] = v[k];
        }
        for (int i = 0; i < n_blocks; i++) { blocks[2 * i] = p->blocks_flat[i].x; blocks[2 * i + 1] = p->blocks_flat[i].y; }
        for (int L = 0; L <= levels; L++) blocks_off[L] = p->blocks_off[L];
        for (int L = 0; L < levels; L++) level_lean[L] = p->level_lean[L];
        return KA_OK;
}

extern "C" int ka_debug_plan(int numseq, const int* lens, int n_tasks, const int* abc, int n_cus, int shared, int cons_K, int hooks,
                             const int* task_ids, int n_ids,
                             int* scalars, int* per_task, int* blocks, int blocks_cap, int* blocks_off, int* level_lean)
{
        if (!lens || !abc || n_cus < 1 || cons_K < 0) return fail("ka_debug_plan: bad arguments");
        if (numseq < 2 || n_tasks < 1 || n_tasks > numseq - 1) return fail("need numseq >= 2 and 1 <= n_tasks <= numseq-1");
        for (int i = 0; i < numseq; i++)
                if (lens[i] < 1) return fail("zero-length sequence (the reference removes them before the dispatcher, msa_check.c:66)");
        KaPlan p;
        read_env(p.env);
        p.n_cus = n_cus; p.shared_gpu = shared != 0; p.cons_K = cons_K; p.test_hooks = hooks;
        const float scal[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };     // (gap penalties and their scaling are no part of the plan)
        if (prepare_tasks(&p, numseq, lens, nullptr, n_tasks, abc, scal)) return KA_FAIL;
        if (task_ids) {
                p.plan_active.assign(n_tasks, 0);
                for (int i = 0; i < n_ids; i++) {
                        if (task_ids[i] < 0 || task_ids[i] >= n_tasks) return fail("task id out of range");
                        p.plan_active[task_ids[i]] = 1;
                }
        }
        if (plan_launches(&p)) return KA_FAIL;
        return export_plan(&p, scalars, per_task, blocks, blocks_cap, blocks_off, level_lean);
}

extern "C" int ka_debug_ctx_plan(ka_ctx* c, int* scalars, int* per_task, int* blocks, int blocks_cap, int* blocks_off, int* level_lean)
{
        if (!c || !c->have_job) return fail("no uploaded job");
        return export_plan(c, scalars, per_task, blocks, blocks_cap, blocks_off, level_lean);
}
