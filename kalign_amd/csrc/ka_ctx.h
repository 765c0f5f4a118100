// ka_ctx.h -- what the host-side translation units of the library share (round 5: ka_api.cpp was one file of 2700 lines): the
// context, the environment switches, the kernel launchers' prototypes, the functions one unit calls in another, the device
// buffer (DevBuf) and the base of the stage handles (KaStage).  Library-internal:
// nothing here is part of the C ABI (include/kalign_amd.h).
//   ka_api.cpp   contexts, upload, the runs (ka_tree_run / _refine / _sync / _download), rows, realignment tree, ka_run_encoded, partial runs
//   ka_plan.cpp  the launch planner: levels, leaf / queued / chained launches, clusters, spare workgroups by a simulated schedule -- over
//                ka_plan.h's KaPlan, the host-only base of the context (no GPU needed: ka_debug_plan); task preparation; ka_tree_upload
//   ka_cons.cpp  anchor consistency (anchors, the N x K batch, position maps), the seq-seq pair batch, the distance batch
//   ka_dist.cpp  one alignment over the GPUs of a node: RCCL loaded at run time, the sharded consistency batch and tree, the in-process transport
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ka_device.h"
#include "ka_plan.h"         // KaEnv, KaPlan (the host-only base of the context), fail()
#include "ka_forest.h"       // the records of the realignment-tree kernels
#include "ka_fam.h"          // the family table's rule and what else the stages of a batch of families share on the host

// the task kernels live in ten translation units (ka_kernels.hip, -DKA_UNIT=0..9); unit 5 is launched through unit 4
extern "C" void ka_unit0_launch(const KaTreeDev* D, const int2* blocks_dev, int nblocks, int chain, hipStream_t stream);   // 8 waves
extern "C" void ka_unit1_launch(const KaTreeDev* D, const int2* blocks_dev, int nblocks, int chain, hipStream_t stream);   // 8 waves + consistency
extern "C" void ka_unit2_launch(const KaTreeDev* D, const int2* blocks_dev, int nblocks, int cons, int nqueue, hipStream_t stream);   // half (4 waves, 2 per CU)
extern "C" void ka_unit3_launch(const KaTreeDev* D, const int2* blocks_dev, int nblocks, int cons, hipStream_t stream);    // lean (seq-seq levels)
extern "C" void ka_unit4_launch(const KaTreeDev* D, const int2* blocks_dev, int nblocks, int cons, hipStream_t stream);    // refinement pass (one workgroup per task)
// the consistency kernels once more with room for ten anchors per DP row (units 6..9; K > KA_NB - 1)
extern "C" void ka_unit6_launch(const KaTreeDev* D, const int2* blocks_dev, int nblocks, int chain, hipStream_t stream);
extern "C" void ka_unit7_launch(const KaTreeDev* D, const int2* blocks_dev, int nblocks, int nqueue, hipStream_t stream);
extern "C" void ka_unit8_launch(const KaTreeDev* D, const int2* blocks_dev, int nblocks, hipStream_t stream);
extern "C" void ka_unit9_launch(const KaTreeDev* D, const int2* blocks_dev, int nblocks, hipStream_t stream);
static inline bool ka_cons_big(const KaTreeDev* D) { return D->cons_K > KA_NB - 1; }
// kind: 0 = 8-wave kernel, 1 = lean (seq-seq only), 2 = half (4 waves, two workgroups per CU)
static inline void ka_launch_task_level(const KaTreeDev* D, const int2* blocks_dev, int nblocks, int kind, int chain, hipStream_t stream)
{
        const int cons = D->cons_K > 0;
        if (ka_cons_big(D)) {
                if (kind == 1) ka_unit8_launch(D, blocks_dev, nblocks, stream);
                else if (kind == 2) ka_unit7_launch(D, blocks_dev, nblocks, 0, stream);
                else ka_unit6_launch(D, blocks_dev, nblocks, chain, stream);
                return;
        }
        if (kind == 1) ka_unit3_launch(D, blocks_dev, nblocks, cons, stream);
        else if (kind == 2) ka_unit2_launch(D, blocks_dev, nblocks, cons, 0, stream);
        else if (cons) ka_unit1_launch(D, blocks_dev, nblocks, chain, stream);
        else ka_unit0_launch(D, blocks_dev, nblocks, chain, stream);
}
extern "C" int ka_max_g_host(void);
extern "C" void ka_launch_posmaps(const int* paths, const long long* poff, const int* pair_of, const int* lens, const long long* map_off,
                                  int numseq, int K, int* maps, hipStream_t stream);
// the realignment tree of a batch of families and the rows of a job (ka_rows.hip; the tables: ka_forest.h)
extern "C" void ka_launch_aln_dist(const uint8_t* rows, long long stride, const KaAdTile* tiles, int n_tiles, const KaAdFam* fams,
                                   const int* fam_of, int numseq, uint8_t gap, float* dm, float* means, hipStream_t stream);
extern "C" int ka_launch_upgma_one_wg(const KaUpgma* table, const int* first, const int* max_n, hipStream_t stream);
extern "C" void ka_launch_upgma(KaUpgma U, hipStream_t stream);                  // one launch per merge
extern "C" void ka_launch_rows(const uint8_t* letters, const int* off, const int* lens, const int* colof, const int* alnlen,
                               int numseq, uint8_t gap, uint8_t* rows, long long stride, const long long* row_off, hipStream_t stream);
int ka_tasks_from_merges(int numseq, const int* merges_ab, int* tasks_abc);      // ka_guide.cpp
double ka_guide_last_dist_ms(void);                                              // ka_guide.cpp: device ms of the distance batches of the last ka_guide_forest
extern "C" void ka_launch_bpm(const uint8_t* codes, const int* off, const int* lens, int numseq, unsigned long long* peq,
                              const int* ia, const int* ib, int npairs, int* dist, hipStream_t stream);
extern "C" long long ka_ctl_bytes_host(void);
extern "C" void ka_launch_pairs(const KaPairDev* P, hipStream_t stream);
extern "C" long long ka_scratch_bytes_host(long long la, long long lb, long long cons_maxlen);
extern "C" long long ka_scratch_bytes_host_big(long long la, long long lb, long long cons_maxlen, long long k_anchors);

#define HIPCHK(x)                                                                         \
        do {                                                                              \
                hipError_t e_ = (x);                                                      \
                if (e_ != hipSuccess) {                                                   \
                        return fail(std::string(#x) + ": " + hipGetErrorString(e_));      \
                }                                                                         \
        } while (0)

// A grow-only device buffer that frees itself with its owner.  An owner that sets its device and waits for its stream does so
// in the body of its destroy function or destructor: the members go after it.  No object with static or thread storage owns
// one (it would free after the runtime is gone), and no pointer of one is handed to something that outlives it.
template <typename T>
struct DevBuf {
        T* p = nullptr;
        size_t n = 0;
        DevBuf() = default;
        DevBuf(const DevBuf&) = delete;
        DevBuf& operator=(const DevBuf&) = delete;
        DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
        DevBuf& operator=(DevBuf&& o) noexcept
        {
                if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
                return *this;
        }
        ~DevBuf() { release(); }
        int alloc(size_t count)
        {
                if (count <= n && p) return 0;
                release();
                if (hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) { p = nullptr; n = 0; return 1; }
                n = count;
                return 0;
        }
        void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

struct ka_ctx;
// the device and the stream of a context (ka_api.cpp); not 0: no context
KA_INTERNAL int ka_ctx_device_stream(ka_ctx* c, int* device, hipStream_t* stream);

// What the handle of a stage of a batch of families (ka_sum_fam, ka_in_fam, ka_cod_fam, ka_out_fam) holds of its context and
// of its calls: device and stream, a few events, and the counters of kernel launches (counted by the launchers) and host waits
// that the stage's *_stats hand out.  Which call resets them, and where they go in st[], is the stage's own.
struct KaStage {
        int device = 0;
        hipStream_t stream = nullptr;
        hipEvent_t ev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
        int nLaunch = 0, nSync = 0;

        KaStage() = default;
        KaStage(const KaStage&) = delete;
        KaStage& operator=(const KaStage&) = delete;
        ~KaStage()
        {
                for (auto& e : ev)
                        if (e) (void)hipEventDestroy(e);
        }
        int attach(ka_ctx* ctx) { return ka_ctx_device_stream(ctx, &device, &stream); }
        // the handle's device made current and its first n events created
        int open(int n)
        {
                HIPCHK(hipSetDevice(device));
                for (int k = 0; k < n; k++) HIPCHK(hipEventCreate(&ev[k]));
                return KA_OK;
        }
        // a call that launches: nothing launched, nothing waited for yet
        void begin() { nLaunch = nSync = 0; }
        // the host waits for the stream: counted where it happens
        int wait()
        {
                HIPCHK(hipStreamSynchronize(stream));
                nSync++;
                return KA_OK;
        }
        // a create that was refused after its uploads went out: nothing of the caller's is read after the refusal
        int refused() { (void)hipStreamSynchronize(stream); return KA_FAIL; }
        float ms(int a = 0, int b = 1) { float m = 0.0f; (void)hipEventElapsedTime(&m, ev[a], ev[b]); return m; }
};

// a stage's destroy: the device, the stream's last work, then the handle and with it its buffers and events
template <typename H>
void ka_stage_destroy(H* h)
{
        if (!h) return;
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        delete h;
}

// The aligned rows that the last rows_build left in d_rows: n rows (0: nothing that a tree can be built from) `stride`
// apart, row i the first alen[i] columns of its tree's alignment, the rest gap.  one_tree: all of one alignment -- what
// ka_aln_guide_tree takes; ka_aln_guide_forest takes any.
struct KaRowsHeld {
        int n = 0;
        long long stride = 0;
        uint8_t gap = 0;
        bool one_tree = false;
        std::vector<int> alen;
        void forget() { n = 0; one_tree = false; }   // a new job, other rows in d_rows
};

// (the switches, the prepared job and its launch plan are the KaPlan base: ka_plan.h)
struct ka_ctx : KaPlan {
        int device = 0;
        hipStream_t stream = nullptr;
        bool own_stream = false;                     // `stream` was created by ka_ctx_set_shared (destroyed with the context)
        // ---- tree job ----
        bool have_job = false;
        int flags = 0;
        std::vector<int> off;
        std::vector<int> level_ids_flat, level_off;
        int refine_mode = 0;                         // the run in flight is a refinement pass (ka_tree_refine / _refine_trees): 1 all, 2 confident
        DevBuf<int2> d_refine_blocks;                   // its workgroup table, level after level (refine_blocks)
        std::vector<int> refine_off;                    // [levels + 1] first block of every level in it
        bool shared_by_fallback = false;             // shared_gpu was forced by a join watchdog (ka_tree_sync), not by the caller
        int fallback_runs = 0;                       // how often that happened (ka_ctx_fallback_runs)
        int fallback_streak = 0;                     // ... on fast-plan jobs in a row (a clean fast-plan run resets it)
        int fallback_hold = 0;                       // jobs that stay on the shared plan before the fast plan is tried again (0 after a first fallback, then 4, 16, 64)
        std::vector<long long> leaf_prof_off;
        long long leaf_prof_total = 0;
        long long sum_len = 0;
        int max_len = 0;
        float subm[23 * 23];
        float scal[6];
        int nres = 23;
        DevBuf<uint8_t> d_codes;
        DevBuf<int> d_seq_off, d_node_len, d_level_ids, d_path_arena, d_error;
        DevBuf<long long> d_node_prof, d_dbg_off, d_timing;
        DevBuf<float> d_prof_arena, d_subm, d_dbg_arena;
        DevBuf<unsigned long long> d_counters;
        DevBuf<char> d_scratch, d_ctl;
        DevBuf<KaJoin> d_join;
        DevBuf<int2> d_blocks;
        DevBuf<KaTaskDesc> d_tasks;
        DevBuf<ka_task_rec> d_recs;
        long long prof_cap = 0, path_cap = 0, scratch_cap = 0, dbg_cap = 0;
        long long scratch_job = 0;                   // what the uploaded job's plan asked of the scratch arena (scratch_cap: what the context holds, never shrinks)
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        std::vector<hipEvent_t> launch_ev;           // KA_LAUNCH_EV: one event behind every launch of the last run
        // two pinned bounce buffers for large downloads into the caller's (pageable) memory
        char* pin[2] = { nullptr, nullptr };
        hipEvent_t pin_ev[2] = { nullptr, nullptr };
        int* h_trace = nullptr;       // pinned, device-visible breadcrumbs (KA_TRACE=1)
        bool ran = false, synced = false;
        bool state_valid = false;      // device state reset and consistent with task_done
        bool partial = false;          // last launch was ka_tree_run_tasks (no automatic grow + re-run)
        std::vector<char> task_done;
        std::vector<char> leaf_written;  // per task, set with task_done: the launch that ran it wrote the records of the sequences it consumes
        // (the first pass writes a sequence's records only for this flag or under sequence weights -- ka_task.h: leaf_syn; a refinement launch always)
        bool first_pass_writes_leaves() const { return (flags & KA_FLAG_LEAF_PROFILES) || scal[5] > 0.0f; }
        std::vector<int> injected;       // nodes whose profile came from ka_tree_set_profile
        DevBuf<int2> d_blocks_tmp;
        // overlapping launches (KA_OVERLAP): the chained launch on a stream of its own (lowest priority) beside the queued launch, events to
        // fork from / join into the context's stream (KaPlan::overlap_plan: the current plan carries the dependencies for it)
        hipStream_t s_chain = nullptr;
        hipEvent_t e_fork = nullptr, e_chain = nullptr;
        int n_launches = 0;
        double cells = 0.0;
        float pair_ms = 0.0f;                        // kernel time of the last ka_pairwise_batch
        // grow-only device buffers of ka_pairwise_batch (no hipMalloc/hipFree per call)
        DevBuf<uint8_t> p_codes; DevBuf<int> p_off, p_len, p_ia, p_ib, p_paths, p_err; DevBuf<float> p_subm, p_scores;
        DevBuf<long long> p_poff; DevBuf<char> p_scr;
        DevBuf<unsigned long long> b_peq; DevBuf<int> b_dist;   // ka_bpm_batch
        std::vector<ka_task_rec> h_recs;
        unsigned long long h_counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        // ---- anchor consistency (ka_tree_build_consistency) ----
        std::vector<uint8_t> h_codes;                // host copy of the uploaded sequences
        std::vector<float> seq_dist;                 // msa->seq_distances (empty: none)
        size_t colof_n = 0;
        bool have_colof = false;       // residue->column tables + member lists are on the device
        float cons_weight = 0.0f;
        std::vector<int> cons_anchor_ids, cons_maps;  // cons_maps: host copy of d_cons_maps, filled on demand
        long long cons_maps_total = 0;
        std::vector<long long> cons_map_off;
        DevBuf<int> d_cons_maps, d_colof, d_colof_init, d_sip, d_alnlen, d_pair_of;
        DevBuf<uint8_t> d_letters, d_rows;
        KaRowsHeld rows;                             // what d_rows holds
        // ---- the realignment trees of a batch of families (ka_aln_guide_forest; one family: a batch of one) ----
        DevBuf<float> d_adm, d_amean; DevBuf<int> d_uactive; DevBuf<unsigned long long> d_ucand; DevBuf<int2> d_umerges;
        DevBuf<KaAdTile> d_adtiles; DevBuf<KaAdFam> d_adfams; DevBuf<int> d_fam_of; DevBuf<KaUpgma> d_utable;
        DevBuf<long long> d_row_off;                 // ka_run_encoded_batch: where every row of a packed hand-out starts
        std::vector<uint8_t> batch_rows;             // the finished rows of the last ka_run_encoded_batch, packed (ka_batch_rows)
        bool have_batch = false;
        double batch_stats[6] = {0, 0, 0, 0, 0, 0};  // ka_batch_stats
        // ka_batch_refine_stats: the last batch's families, whether it ran refine_mode 2, and then per family the threshold,
        // the tasks and the marked tasks
        int batch_n_fam = 0;
        bool batch_confident = false;
        std::vector<float> batch_thr;
        std::vector<int> batch_edges, batch_refined;
        DevBuf<long long> d_cons_map_off, d_sip_off;
};

KA_INTERNAL int upload_plan(ka_ctx* c);
KA_INTERNAL int setup_colof(ka_ctx* c);
KA_INTERNAL int refine_blocks(ka_ctx* c, int mode);
KA_INTERNAL int pairwise_on_device(ka_ctx* c, const uint8_t* codes, const int* off, const int* lens, int numseq,
                              const int* ia, const int* ib, int npairs,
                              const float* subm, float gpo, float gpe, float tgpe, const long long* poff, long long* ptotal_out);
KA_INTERNAL void node_members(const ka_ctx* c, int node, long long* lo, long long* hi);

KA_INTERNAL int copy_to_host(ka_ctx* c, void* dst, const void* src, size_t bytes);
KA_INTERNAL int tree_reset(ka_ctx* c);
KA_INTERNAL KaTreeDev tree_dev(ka_ctx* c);
KA_INTERNAL int tree_launch(ka_ctx* c, bool reset = true);

