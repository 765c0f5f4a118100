// ka_plan.h -- the host-only part of a context: the KA_* switches, the prepared job (task descriptors, levels) and its launch plan.
// Nothing here holds a device handle: a KaPlan is filled and planned without a GPU (ka_debug_plan, tests/test_plan_host.py), and
// the planner (ka_plan.cpp: prepare_tasks, plan_launches, build_blocks) sees a context only as this base of it.
#pragma once
#define KA_INTERNAL __attribute__((visibility("hidden")))

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "ka_device.h"

// the thread's error text (ka_last_error) and the one way to set it: defined in ka_api.cpp
KA_INTERNAL int fail(const std::string& m);

// The KA_* environment switches (experiments, measurements and tests; none is needed in production), read ONCE when the
// context is created -- ka_debug_reload_env re-reads them for tools and tests that flip a switch on a live context.
struct KaEnv {
        bool trace = false, no_chain = false, no_queue = false, no_half = false, no_lean = false, chain_g1 = false, no_crit = false;
        bool no_staging = false, no_wdfs = false, no_ls0 = false, no_inc = false, no_ldfs = false, refine_serial = false;
        int chain_tasks = 0;           // KA_CHAIN_TASKS: the chained launch starts at the first level with at most this many tasks (0: CUs - 8)
        int max_cluster = 0;           // KA_MAX_CLUSTER: workgroups one task may use (0: the default, 16)
        int crit_greedy = 1;           // KA_CRIT_GREEDY: spare chain workgroups by a simulated schedule first (0: by the ranking alone)
        int crit_top = 0;              // KA_CRIT_TOP: workgroups of the chain entry with the longest way to the root (0: default)
        int prof_task = -1;            // KA_PROF_TASK: the task whose per-level times KA_FLAG_TIMING keeps (-1: the root)
        int q1 = -1;                   // KA_Q1 (-1: the default -- 4 for protein jobs: 64-row strips per recursion level where every strip still gets a helper wave, 0 for nucleotides): 64-row strips (KaTreeDev::q1_mode); measured no faster with 64-column hand-over batches (round 3)
        int lean4 = 1;                 // KA_LEAN4: leaf levels on 4-wave workgroups, four per CU (1.60 -> 1.28 ms on the 4096 x 400 leaf level)
        int mw = 1;                    // KA_MW: multi-wave scan of the top-level meetups
        int merge = 15;                // KA_MERGE: ka_update_profile in batches (bit 0: operands with records in HBM, bit 1: sequences too, bit 2: clusters too, bit 3: the seq-seq tasks of the 128-register units)
        int per = 0;                   // KA_PER: strips per workgroup (KaTreeDev::per_target; experiments)
        int ho = -1;                   // KA_HO: hand-over between neighbouring strips through LDS (KaTreeDev::ho_mode); -1: on (1)
        int hw = 1;                    // KA_HW: profile-profile strips with helper waves (ka_wstrip.h; KaTreeDev::hw_mode)
        int sparse = 1;                // KA_SPARSE: profile-profile strips whose rows have few non-zero counts run the gathered dot product (ka_pass.h; KaTreeDev::sparse_mode); 0: every strip dense
        int hw_prio = 3;               // KA_HW_PRIO: s_setprio of a strip wave that has a helper (experiments)
        int subtree = 1;               // KA_SUBTREE: small Hirschberg subtrees run wave-locally in LDS
        int overlap = 1;               // KA_OVERLAP: the chained launch goes out beside the queued launch (a stream of its own, ordered by the tasks' done flags)
        int overlap_help = 1;          // KA_OVERLAP_HELP: workgroups of the chained launch that arrive before the queue's last round take queue tasks
        int reuse = 1;                 // KA_REUSE: Hirschberg prefix reuse in the 4-wave kernels (queued levels, seq-seq leaves, pair batch)
        int qw = 4, lw = 4, pw = 2;    // KA_QW / KA_LW / KA_PW: waves per workgroup of the queued launch, the seq-seq leaf levels, the pair batch (4, 2, 1)
        bool launch_ev = false;        // KA_LAUNCH_EV: an event behind every launch of a run (ka_tree_launch_ms)
        bool upgma_launches = false;   // KA_UPGMA_LAUNCHES: ka_aln_guide_tree's UPGMA as one launch per merge (the path for > 6144 sequences) at any size
        bool qorder = true;            // KA_QORDER: the queue's order -- 0 list order, anything else per level by the way to the root
        bool plan_verbose = false;     // KA_PLAN_VERBOSE: the chained launch's plan on stderr
};
static inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static inline void read_env(KaEnv& v)
{
        v = KaEnv();
        v.trace = getenv("KA_TRACE") != nullptr; v.no_chain = getenv("KA_NO_CHAIN") != nullptr; v.no_queue = getenv("KA_NO_QUEUE") != nullptr;
        v.no_half = getenv("KA_NO_HALF") != nullptr; v.no_lean = getenv("KA_NO_LEAN") != nullptr; v.chain_g1 = getenv("KA_CHAIN_G1") != nullptr;
        v.no_crit = getenv("KA_NO_CRIT") != nullptr; v.no_staging = getenv("KA_NO_STAGING") != nullptr;
        v.no_wdfs = getenv("KA_NO_WDFS") != nullptr; v.no_ls0 = getenv("KA_NO_LS0") != nullptr; v.no_inc = getenv("KA_NO_INC") != nullptr; v.no_ldfs = getenv("KA_NO_LDFS") != nullptr; v.refine_serial = getenv("KA_REFINE_SERIAL") != nullptr;
        v.chain_tasks = env_int("KA_CHAIN_TASKS", 0); v.max_cluster = env_int("KA_MAX_CLUSTER", 0); v.crit_top = env_int("KA_CRIT_TOP", 0); v.crit_greedy = env_int("KA_CRIT_GREEDY", 1);
        v.prof_task = env_int("KA_PROF_TASK", -1); v.q1 = env_int("KA_Q1", -1); v.lean4 = env_int("KA_LEAN4", 1);
        v.launch_ev = getenv("KA_LAUNCH_EV") != nullptr;
        v.subtree = env_int("KA_SUBTREE", 1);
        v.reuse = env_int("KA_REUSE", 1);
        v.overlap_help = env_int("KA_OVERLAP_HELP", 1);
        v.overlap = env_int("KA_OVERLAP", 1);
        v.qw = env_int("KA_QW", 4); v.lw = env_int("KA_LW", 4); v.pw = env_int("KA_PW", 2);
        for (int* w : { &v.qw, &v.lw, &v.pw }) if (*w != 1 && *w != 2) *w = 4;
        v.mw = env_int("KA_MW", 1);
        v.merge = env_int("KA_MERGE", 15);
        v.ho = env_int("KA_HO", -1);
        v.per = env_int("KA_PER", 0);
        v.hw = env_int("KA_HW", 1);
        v.sparse = env_int("KA_SPARSE", 1);
        v.hw_prio = std::max(0, std::min(3, env_int("KA_HW_PRIO", 3)));
        v.upgma_launches = getenv("KA_UPGMA_LAUNCHES") != nullptr;
        v.qorder = env_int("KA_QORDER", 1) != 0;
        v.plan_verbose = getenv("KA_PLAN_VERBOSE") != nullptr;
}

struct KaPlan {
        KaEnv env;
        // ---- the job, as prepare_tasks leaves it ----
        int numseq = 0, n_tasks = 0;
        std::vector<int> lens;
        std::vector<int> abc;
        std::vector<KaTaskDesc> descs;               // (the plan sets parent, chain_need, is_root, wait_mult, qa, qb of every task)
        std::vector<std::vector<int>> levels;        // task ids per dependency level
        std::vector<int> task_level;
        std::vector<int> sip_flat;                   // member lists of every node, reference order
        std::vector<long long> sip_off;
        // ---- what else the plan depends on ----
        std::vector<char> plan_active;               // the tasks it covers (empty: the whole job) -- ka_tree_plan_tasks
        int n_cus = 256;                             // compute units of the device (hipDeviceProp)
        bool shared_gpu = false;                     // ka_ctx_set_shared: no multi-workgroup tasks, no chained launch
        int cons_K = 0;                              // anchors of the consistency table (0: none)
        int test_hooks = 0;                          // ka_debug_set_hooks (tests only)
        // ---- the plan (plan_launches) ----
        std::vector<std::vector<int>> plan_levels;   // `levels` of the tasks the current launch plan covers
        std::vector<int2> blocks_flat;               // per level: (task, member | cluster size << 8) per workgroup
        std::vector<int> blocks_off;
        std::vector<int> level_lean;                 // level consists of seq-seq tasks only -> lean kernel
        int max_cluster = 16;                        // KA_MAX_CLUSTER env: workgroups (CUs) one task may use
        int n_trees = 1;               // guide trees in the job (a forest when > 1)
        int chain_level = -1;          // first level of the chained launch (-1: every level is its own launch)
        int queue_first = -1;          // queued launch: levels queue_first .. chain_level-1 run as ONE launch of the half kernel (-1: none)
        int queue_off = 0, queue_n = 0; // its task list in blocks_flat
        int overlap_plan = 0;          // the plan carries the dependencies for overlapping launches (KA_OVERLAP)
        std::vector<int2> chain_blocks;
        int chain_blocks_off = 0;
};

// Host-side task preparation of ka_tree_upload: order checks, nsip, sip lists, gap_scale / subm_offset, levels.  seq_distances may be null.
KA_INTERNAL int prepare_tasks(KaPlan* p, int numseq, const int* lens, const float* seq_distances, int n_tasks, const int* abc, const float* scal);
KA_INTERNAL void build_blocks(const KaPlan* p, const std::vector<int>& L, std::vector<int2>& tbl, int* lean_out);
KA_INTERNAL int plan_launches(KaPlan* p);
