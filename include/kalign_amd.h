/*
 * kalign_amd.h -- C ABI of the MI355X (gfx950) implementation of Kalign's
 * progressive-alignment hot path: the batched seq-seq / seq-profile /
 * profile-profile affine-gap Gotoh DP under a linear-space Hirschberg
 * recursion, and the guide-tree task dispatcher that feeds it.
 *
 * The seam this replaces in the reference (TimoLassmann/kalign v3.5.1) is
 * link-time and in-process:
 *
 *   ka_msa_tree()        <->  create_msa_tree(struct msa*, struct aln_param*, struct aln_tasks*)
 *                              lib/src/aln_run.c:43-78, with do_align :213-441 per task
 *   ka_pairwise_batch()  <->  the N x K loop over pairwise_align_map() -> aln_runner()
 *                              lib/src/anchor_consistency.c:19-120, :246-267
 *   ka_tree_build_consistency() <-> anchor_consistency_build(), lib/src/anchor_consistency.c:194-275, plus the
 *                              per-task bonus of do_align (aln_run.c:262-295) inside ka_tree_run
 *   ka_tree_upload/run/download: the same dispatcher split so that a caller can
 *                              keep inputs resident in HBM (bench.py times ka_tree_run only)
 *
 * All pointers are plain host pointers unless a name says "dev".  Return
 * value 0 = OK, non-zero = FAIL (the reference's convention, tldevel.h:29-45);
 * ka_last_error() gives a message.  INTEGRATION.md shows the exact glue a
 * Kalign maintainer adds in aln_run.c / anchor_consistency.c.
 *
 * Sequence encoding is the reference's internal alphabet (alphabet.c:179-245):
 * protein 0..22, nucleotide 0..4.  Profiles use the reference's 64-float record
 * layout (aln_setup.c:40-99).  Paths are the reference's coded paths
 * (add_gap_info_to_path_n, aln_setup.c:121-228): p[0] = alignment length,
 * p[1..len] ops (0 match, 1 gap in a, 2 gap in b, |32 terminal run), p[len+1] = 3.
 */
#ifndef KALIGN_AMD_H
#define KALIGN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KA_OK 0
#define KA_FAIL 1
#define KA_ERR_PATHS_CAP 2      /* caller's paths_out too small; required size in ka_tree_paths_size() */
#define KA_ERR_ROWS_STRIDE 3    /* ka_run_encoded: rows_out too narrow; alnlen_out holds the length, the alignment is still on the device */

/* flags for ka_msa_tree / ka_tree_upload */
#define KA_FLAG_DEBUG_ROWS 1    /* also keep each task's top-level f/b rows (tests: row hashes) */
#define KA_FLAG_TIMING 2        /* record per-task phase cycle counts (ka_tree_get_timing) */
#define KA_FLAG_DEVICE_GAPS 4   /* keep every residue's alignment column on the device (make_seq / update_gaps,
                                   weave_alignment.c:41-112): ka_tree_download derives gaps_out from it in O(sum of
                                   lengths) instead of folding every task's path on the host; ka_msa_tree sets it
                                   when gaps_out is requested */
#define KA_FLAG_KEEP_CONSISTENCY 8 /* the realignment pass of kalign_run_realign (aln_wrap.c:424-431,497-502): the same
                                   sequences with a new task list keep the consistency table ka_tree_build_consistency
                                   built for the previous job of this context (no table then: none now); fails if the
                                   sequences differ */
#define KA_FLAG_EXACT_CONFIDENCE 16 /* task confidence as the reference's float, bit for bit: the reference adds a task's meetup
                                   margins in recursion order (aln_run.c:391-395, aln_controller.c:194-436), the level-synchronous
                                   first pass in level order (equal within 1e-5).  With this flag every meetup records its margin with
                                   its place in the recursion order; sorted and added in fp32 after the recursion.  Costs a sort per
                                   task and the wave-local subtrees (the records are not kept there); tasks with more than 8192
                                   recorded meetups keep the level-order sum. */
#define KA_FLAG_LEAF_PROFILES 32 /* also write the profile records of the SEQUENCES (make_profile_n, aln_setup.c:40-99) that tasks consume.  Since
                                   round 6 the first pass does not (without sequence weights): a sequence's record is a function of its
                                   residue, and the merge makes what it needs of it on the fly -- ka_tree_get_profile and ka_tree_profile_dev
                                   of a node < numseq then FAIL (ABI 21; before, they returned unwritten memory).  Set this to read leaf
                                   profiles back.  They succeed as well with sequence weights (scal[5] > 0) and after ka_tree_refine, which
                                   write the records -- in every case only once the task that consumes the sequence has run: the records
                                   carry that task's penalties and score offset. */

typedef struct ka_ctx ka_ctx;

/* Per-task result; field-for-field what do_align leaves behind plus the top-level
   Hirschberg meetup (aln_controller.c:21-120).  Same layout as the oracle's ko_task_rec. */
typedef struct ka_task_rec {
        int a, b, c;            /* task (a, b) -> c, struct task (task.h:14-22) */
        int len_a, len_b;       /* operand lengths in (a, b) order */
        int nsip_a, nsip_b;     /* member counts, msa->nsip[] */
        int plen;               /* alignment length, msa->plen[c] */
        int kind;               /* 0 seq-seq, 1 seq-profile, 2 profile-profile */
        int swapped;            /* DP ran with b as rows (aln_run.c:297-388 swap rules) */
        int meet, transition;   /* top-level meetup column / transition code 1,2,3,5,6,7 */
        int path_off;           /* offset of this task's coded path in paths_out */
        float gap_scale;        /* compute_gap_scale (aln_run.c:126-164) */
        float subm_off;         /* compute_subm_offset (aln_run.c:166-203) */
        float score;            /* top-level meetup score (== m->score of ALN_MODE_SCORE_ONLY) */
        float confidence;       /* mean Hirschberg margin, task.confidence (aln_run.c:391-395) */
        uint64_t prof_hash;     /* FNV-1a of the merged profile bytes, 0 for the root / when not requested */
        uint64_t fhash, bhash;  /* FNV-1a of top-level f / b rows (KA_FLAG_DEBUG_ROWS), else 0 */
} ka_task_rec;

int  ka_ctx_create(int device, ka_ctx** out);
void ka_ctx_destroy(ka_ctx* ctx);
/* Launch on the caller's HIP stream (a hipStream_t, e.g. torch's current stream). NULL = default stream. */
int  ka_ctx_set_stream(ka_ctx* ctx, void* hip_stream);
/* Tell the context that it does NOT have the GPU to itself (several alignments in flight on different streams /
   processes).  Multi-workgroup tasks and the chained launch make workgroups wait for each other and need all of
   them resident; a shared context runs every task on one workgroup, one launch per guide-tree level -- slower for
   a single tree, safe under any co-scheduling.  Takes effect at the next ka_tree_upload.  A shared context that was
   given no stream (ka_ctx_set_stream) creates a non-blocking stream of its own: contexts of one process that stay on
   the null stream run one after the other however many host threads drive them. */
int  ka_ctx_set_shared(ka_ctx* ctx, int shared);
/* How often a run of this context fell back to that plan on its own because a wait between workgroups never
   completed (another process was using the GPU): the run is repeated and correct, but slower -- visible here. */
int  ka_ctx_fallback_runs(ka_ctx* ctx);
/* Bytes of device memory in the context's profile, path and scratch arenas.  They grow to the largest job the context has
   seen (and on overflow) and are kept from job to job; a job of a shape the context has already run leaves them as they are. */
long long ka_ctx_arena_bytes(ka_ctx* ctx);
/* Of the last finished run: tasks of the queued launch that workgroups of the chained launch took over because they were resident
   before the queue was down to its last round (overlapping launches; normally 0).  -1: nothing finished. */
long long ka_ctx_helped_tasks(ka_ctx* ctx);
const char* ka_last_error(void);
/* ABI revision of this header (bumped when entry points are added) */
int  ka_abi_version(void);

/*
 * The dispatcher.  numseq sequences (concatenated codes, off[i], lens[i]),
 * n_tasks = numseq-1 tasks in TASK_ORDER_TREE order (children before parents,
 * root last; task.c:114-136) as abc[3*t + {0,1,2}].
 * subm: 23*23 floats; scal[6] = gpo, gpe, tgpe, dist_scale, vsm_amax, use_seq_weights
 * (struct aln_param, aln_param.h:19-34, after the sentinel resolution of aln_param_init).
 * seq_distances: numseq floats or NULL (msa->seq_distances).
 * n_tasks < numseq-1 describes a FOREST: several independent alignments (a batch of families, ensemble members)
 * scheduled together -- node ids stay unique, every task nobody consumes is the root of its tree, and the
 * levels of all trees share launches (the GPU is mostly idle at the top of a single tree).
 * Outputs: recs[n_tasks]; coded paths packed into paths_out (capacity paths_cap ints);
 * gaps_out: concatenated gaps[len+1] per sequence (msa->sequences[i]->gaps after make_seq,
 * weave_alignment.c:41-112) or NULL.
 */
int ka_msa_tree(ka_ctx* ctx, int numseq, const uint8_t* codes, const int* off, const int* lens,
                const float* seq_distances, int n_tasks, const int* tasks_abc,
                const float* subm, const float* scal, int flags,
                ka_task_rec* recs, int* paths_out, long long paths_cap, int* gaps_out);

/* The same, staged: upload (H2D + host-side task preparation), run (device only; may be
   called repeatedly -- it resets the device state first), download (D2H + gap weaving). */
int ka_tree_upload(ka_ctx* ctx, int numseq, const uint8_t* codes, const int* off, const int* lens,
                   const float* seq_distances, int n_tasks, const int* tasks_abc,
                   const float* subm, const float* scal, int flags);
int ka_tree_run(ka_ctx* ctx);
/* refine_alignment (aln_refine.c:34-85): a second pass over every edge of the uploaded tree with refine_edge's flip
   trials (aln_refine.c:199-325: trial 0 is the baseline, trials 1-4 take the second-best meetup round-robin where the
   margin is below the baseline's mean margin; the trial with the best sum-of-pairs score is kept, the first one on
   ties).  mode 1 = KALIGN_REFINE_ALL, 2 = KALIGN_REFINE_CONFIDENT (only edges whose first-pass confidence is at or
   below the median are refined, the others are re-aligned plainly), 3 = KALIGN_REFINE_INLINE
   (create_msa_tree_inline_refine, aln_run.c:448-790, as aln_wrap.c:222-224 calls it: one pass, three trials on every
   edge, first-pass path coding, task confidence = the kept trial's sum-of-pairs score), 4 = no refinement: the first
   pass again, run depth first like the reference so that every task's confidence is the reference's exact float sum
   (ka_tree_run adds the same margins level by level: equal within 1e-5).  conf_in[n_tasks]: first-pass task
   confidences (the reference reads task->confidence); only read for mode 2; NULL = computed here with a mode-4 pass.  Asynchronous like
   ka_tree_run; ka_tree_sync / ka_tree_download then return the refined records, paths and gaps (records carry the
   kept trial's confidence).
   On a forest job ka_tree_refine takes mode 2's median POOLED, over all tasks of the job whatever tree they are of;
   ka_tree_refine_trees (below) takes it per tree, which is what the reference does with each alignment. */
#define KA_REFINE_ADAPTIVE 256      /* mode | KA_REFINE_ADAPTIVE: aln_param's adaptive_budget (`kalign --adaptive-budget`,
                                       aln_refine.c:187-193, 255-282; modes 1 and 2): 1 .. 8 trials per edge, from the share of
                                       very uncertain meetups of its baseline trial */
#define KA_REFINE_TRIALS(n) (((n) & 255) << 16)   /* 3 | KA_REFINE_TRIALS(n): create_msa_tree_inline_refine with n trials per edge
                                                     (lib/src/aln_run.c:448-475 takes any count; kalign_run passes 3, the default here) */
int ka_tree_refine(ka_ctx* ctx, int mode, const float* conf_in);
/* ka_tree_refine with mode 2's rule per TREE of the job: same modes, flags, conf_in and asynchrony; on a job of one tree the
   same call.  A tree is the set of tasks that lead to one root (a task nobody consumes), trees are numbered by ascending
   index of their root task, and a tree of n tasks has compute_confidence_threshold's threshold (aln_refine.c:674-712) of
   its own n confidences: sorted ascending, v[n/2] for odd n, (v[n/2-1] + v[n/2]) / 2.0F in fp32 for even n; an edge is
   refined when its confidence is <= its tree's threshold (a tree of one task always).  The trees are read from the task
   list alone, so their tasks may be interleaved.
     tree_of_out[n_tasks]  (may be NULL) the tree of every task
     thr_out[n_tasks]      (may be NULL) room for n_tasks values, the first n_trees filled: every tree's threshold (0 in modes 1, 3, 4)
     n_trees_out           (may be NULL) */
int ka_tree_refine_trees(ka_ctx* ctx, int mode, const float* conf_in, int* tree_of_out, float* thr_out, int* n_trees_out);
int ka_tree_sync(ka_ctx* ctx);
long long ka_tree_paths_size(ka_ctx* ctx);      /* ints needed for paths_out (valid after run+sync) */
int ka_tree_download(ka_ctx* ctx, ka_task_rec* recs, int* paths_out, long long paths_cap, int* gaps_out);

/* The aligned rows themselves (finalise_alignment + make_linear_sequence, lib/src/msa_op.c:546-598), built on the
 * device from the residue->column tables of a job uploaded with KA_FLAG_DEVICE_GAPS, after a complete run.
 *   letters[sum of lens]  the residues as the caller wants them printed (struct msa_seq.seq), laid out like `codes`
 *   rows_out[numseq * row_stride]  row i holds alnlen(i) bytes -- letters, and gap_char where the reference puts
 *                         '-' -- followed by a 0 byte; row_stride >= the longest alignment + 1
 *   alnlen_out[numseq]    (may be NULL) alignment length of the tree sequence i belongs to (struct msa.alnlen)
 * rows_out == NULL: only alnlen_out is filled (size query). */
int ka_tree_aligned_rows(ka_ctx* ctx, const uint8_t* letters, uint8_t gap_char, uint8_t* rows_out,
                         long long row_stride, int* alnlen_out);
/*
 * Partial runs -- what single-tree multi-GPU sharding is made of (kalign_amd/dist.py:sharded_tree
 * drives them with one process per GPU): a rank runs the tasks of its subtree, the profile of a subtree root moves
 * to the rank that runs its parent (ka_tree_get_profile -> send/recv -> ka_tree_set_profile), rank 0 gathers all
 * records and paths and weaves the gap arrays.  Results do not depend on the number of ranks.
 *   ka_tree_run_tasks: run the listed tasks (children must be available here: leaves, earlier tasks, injected
 *     profiles); does not reset the device state (ka_tree_upload / ka_tree_run do).
 *   ka_tree_reset: forget every computed / injected node (a new sharded run over the same upload).
 *   ka_tree_node_len: alignment length of a node on this context (-1 on error).
 *   ka_tree_set_profile: inject the merged profile of an internal node, (plen+2)*64 floats.
 *   ka_tree_get_node_cols / ka_tree_set_node_cols: with a consistency table, the residue -> column table of the
 *     node's member sequences (ka_tree_node_cols_size ints) travels with the profile.
 *   ka_tree_download_tasks: records + coded paths of the listed tasks, paths packed in list order.
 *   ka_weave_gaps: host-only make_seq/update_gaps over all tasks in tree order (weave_alignment.c:41-112);
 *     recs[t] needs a, b, c, path_off.
 */
int ka_tree_run_tasks(ka_ctx* ctx, const int* task_ids, int n);
/* The listed tasks as ONE planned run -- queued and chained launches where they apply, like a whole tree (what a rank of
 * a sharded tree does with its subtrees; ka_tree_run_tasks launches level by level).  The set must be closed under
 * descendants among the tasks not run yet.  task_ids == NULL plans the whole tree again (ka_tree_run does that itself).
 * ka_tree_run_planned runs the planned tasks on top of what the context holds; no reset. */
int ka_tree_plan_tasks(ka_ctx* ctx, const int* task_ids, int n);
int ka_tree_run_planned(ka_ctx* ctx);
/* The same hand-over without the host: ka_tree_profile_dev says where the (plen+2)*64 floats of a node's profile lie in
 * this context's HBM, ka_tree_reserve_profile_dev reserves room for an incoming profile of `plen` columns on the
 * receiving context and makes the node available to ka_tree_run_tasks; the caller moves the bytes device to device
 * (RCCL send / recv over xGMI -- kalign_amd/dist.py -- or hipMemcpyPeer) before it runs the parent. */
int ka_tree_profile_dev(ka_ctx* ctx, int node, void** dev_ptr, int* plen_out);
int ka_tree_reserve_profile_dev(ka_ctx* ctx, int node, int plen, void** dev_ptr);
int ka_tree_reset(ka_ctx* ctx);
int ka_tree_node_len(ka_ctx* ctx, int node);
int ka_tree_set_profile(ka_ctx* ctx, int node, const float* prof, int plen);
long long ka_tree_node_cols_size(ka_ctx* ctx, int node);
int ka_tree_get_node_cols(ka_ctx* ctx, int node, int* out);
int ka_tree_set_node_cols(ka_ctx* ctx, int node, const int* cols);
int ka_tree_download_tasks(ka_ctx* ctx, const int* task_ids, int n, ka_task_rec* recs, int* paths_out,
                           long long paths_cap, long long* used_out);
int ka_weave_gaps(int numseq, const int* lens, int n_tasks, const ka_task_rec* recs, const int* paths, int* gaps_out);
/* After a run made elsewhere (a sharded tree: records gathered, gap arrays woven on the host) this context -- same uploaded
 * job -- becomes the holder of the finished alignment: recs[n_tasks] (plen, c) and gaps (ka_tree_download's layout) in;
 * ka_tree_aligned_rows, ka_aln_guide_tree and ka_tree_refine then carry on here as after ka_tree_run + ka_tree_sync
 * (finalise_alignment msa_op.c:546-598, refine_alignment aln_refine.c:36-88, compute_aln_pairwise_dist aln_apair_dist.c:9-86). */
int ka_tree_adopt_alignment(ka_ctx* ctx, const ka_task_rec* recs, const int* gaps);

/* Merged profile of node `node` ((plen+2)*64 floats) after a run.  A sequence (node < numseq): see KA_FLAG_LEAF_PROFILES. */
int ka_tree_get_profile(ka_ctx* ctx, int node, float* out, long long cap_floats);
/* Per-task phase timings of the last run (KA_FLAG_TIMING): out[8*t + k], shader-clock cycles:
   0 operand prep, 1 Hirschberg, 2 path coding, 3 profile merge, 4 passes, 5 meetups, 6 recursion
   levels | workgroups used << 8 | workgroups offered << 16, 7 DP rows*cols; followed by 16 x (sub-problems, pass cycles, meetup cycles) per
   recursion level of the root task, followed by 512 values that only profiling builds (-DKA_PROF) fill:
   out must hold 8*n_tasks + 48 + 512 values. */
int ka_tree_get_timing(ka_ctx* ctx, long long* out);
/* Tests only -- fault injection for the recovery paths of ka_tree_sync (takes effect at the next ka_tree_upload):
   KA_DEBUG_SMALL_ARENAS starts with device arenas that are certainly too small (overflow -> grow -> re-run),
   KA_DEBUG_STARVE_ROOT_JOIN makes the root's join wait for a workgroup that never comes (watchdog -> re-plan). */
#define KA_DEBUG_SMALL_ARENAS 1
#define KA_DEBUG_STARVE_ROOT_JOIN 2
#define KA_DEBUG_STARVE_REFINE_MEMBER 4   /* ka_tree_refine: a member of the first multi-workgroup edge never starts (watchdog -> re-plan) */
#define KA_DEBUG_CHAIN_FIRST 8            /* overlapping launches: the chained launch is enqueued BEFORE the queued one -- its workgroups take the CUs
                                             first, as a dispatcher that ignores the streams' priorities would have it (they help the queue) */
#define KA_DEBUG_POISON_ARENAS 16         /* every run starts with the profile, scratch and path arenas filled with 0xff bytes (NaN / -1): nothing may
                                             depend on what an arena held before (round 6: sequences' profile records are no longer written) */
int ka_debug_set_hooks(ka_ctx* ctx, int hooks);
/* Tools and tests: the KA_* environment switches (experiments and measurements; none is needed in production) are read
   once, at ka_ctx_create.  This reads them again and rebuilds the launch plan of the uploaded job. */
int ka_debug_reload_env(ka_ctx* ctx);
/* Tests and tools, no GPU and no context: the launch plan the library would make for a job -- task preparation and planner exactly as
 * ka_tree_upload runs them, on a device of n_cus compute units, with ka_ctx_set_shared(shared), a consistency table of cons_K anchors
 * (0: none), the ka_debug_set_hooks bits `hooks`, and, where task_ids is not NULL, for that subset of the tasks as ka_tree_plan_tasks
 * plans it.  The KA_* switches are read from the environment on every call.  The plan comes back flattened:
 *   scalars[16]            0 levels, 1 entries of the block table, 2 workgroups one task may use, 3 trees, 4 first level of the chained
 *                          launch (-1: none), 5 first level of the queued launch (-1: none), 6 / 7 the queue's list in the block table
 *                          (first entry, entries), 8 overlapping launches, 9 / 10 the chained launch's table in the block table
 *                          (first entry, entries; 0, 0 without one), 11 .. 15 zero
 *   per_task[6 * n_tasks]  parent, chain_need, is_root, wait_mult, qa, qb of every task
 *   blocks[2 * entries]    the block table, (task, member | cluster size << 8) per workgroup: one table per level, the queue's
 *                          list, the chained launch's table
 *   blocks_off[levels + 1] first entry of every level's table;  level_lean[levels]: its launch kind (0 eight waves, 1 lean, 2 half)
 * blocks_off and level_lean must hold n_tasks + 1 and n_tasks values.  With more than blocks_cap entries the call fails after it has
 * filled scalars: call again with room for scalars[1] entries. */
int ka_debug_plan(int numseq, const int* lens, int n_tasks, const int* tasks_abc, int n_cus, int shared, int cons_K, int hooks,
                  const int* task_ids, int n_ids,
                  int* scalars, int* per_task, int* blocks, int blocks_cap, int* blocks_off, int* level_lean);
/* ... and, flattened in the same way, the plan a context holds after ka_tree_upload, ka_tree_plan_tasks or ka_debug_reload_env. */
int ka_debug_ctx_plan(ka_ctx* ctx, int* scalars, int* per_task, int* blocks, int blocks_cap, int* blocks_off, int* level_lean);
/* Tests, no GPU and no context: the edges a mode-2 refinement pass marks, by the function ka_tree_refine(_trees) calls.  The task list
 * as ka_tree_upload takes it (a forest's trees may be interleaved), a confidence per task; pooled != 0: ka_tree_refine's one median
 * over all tasks, which every tree then has as its threshold; 0: ka_tree_refine_trees' median per tree.  tree_of_out[n_tasks],
 * thr_out[n_tasks] (the first *n_trees_out filled), marks_out[n_tasks] (1: conf <= the tree's threshold).  A list that ka_tree_upload
 * would not take is refused with the cause and the task ("children before parents", "a node is consumed twice"). */
int ka_debug_refine_marks(int numseq, int n_tasks, const int* tasks_abc, const float* conf, int pooled,
                          int* tree_of_out, float* thr_out, int* marks_out, int* n_trees_out);
/* Debug: 64 breadcrumb words written by workgroup 0 (context created with KA_TRACE=1 in the
   environment); readable while a kernel is still running. */
int ka_debug_trace(ka_ctx* ctx, int* out64);
/* Tests only: ONE level of the device 2-means bisection (ka_kmeans.hip), launched by the function the product's level loop
 * calls, with everything it computed handed back candidate by candidate.  dm[numrows][32]: distances to the 32 anchors;
 * samples[n_samples]: the level's sample buffer (row indices); sets_start_n[2 * n_sets]: the sets to split, (start, n)
 * slices of it, n >= 2.  force_big != 0: the 512-thread shape whatever the sizes (the product takes it for every set of a
 * level that holds one above 1024 samples).  Set k has tries_k = min(40, n_k) candidates (seed c * (n_k / tries_k)); with
 * slot = sum of tries before k + c and B = sum of tries_j * n_j before k + c * n_k:
 *   score[slot], counts[2 * slot + {0, 1}] = n_left, n_right; lists[2 * B ..]: n_k ints of the left list, then n_k of the
 *   right one (valid up to their counts); mind[B ..]: n_k floats, min(dl, dr) of every sample in the candidate's last
 *   iteration; wmean[32 * k ..]: the set's centroid; winner[k]: the candidate the acceptance rule picks;
 *   *big_out (may be NULL): whether the 512-thread shape ran. */
int ka_debug_kmeans_level(ka_ctx* ctx, const float* dm, int numrows, const int* samples, int n_samples,
                          const int* sets_start_n, int n_sets, int force_big,
                          float* score, int* counts, int* lists, float* mind, float* wmean, int* winner, int* big_out);
/* Tests only, no GPU: the host's split2 (ka_guide.cpp) on the set samples[n] from the seed samples[seed_pick]:
 * *score, counts[2], lists[2 * n] (left list at 0, right list at n), mind[n] and wmean[32] as above, counters[4] =
 * iterations run, samples decided by the index parity rule summed over all iterations, the same in the last iteration,
 * whether the degenerate cut (one side empty) was taken. */
int ka_debug_kmeans_host(const float* dm, int numrows, const int* samples, int n, int seed_pick,
                         float* score, int* counts, int* lists, float* mind, float* wmean, int* counters);
/* Work done by the last run: sum over tasks of len_a*len_b ("useful cells") */
double ka_tree_cells(ka_ctx* ctx);
/* Milliseconds spent in the DP kernels of the last ka_tree_run, measured with HIP events
   on the launch stream; n_launches receives the number of kernel launches. */
int ka_tree_kernel_ms(ka_ctx* ctx, float* ms, int* n_launches);
/* Measurements: the duration of every launch of the last run (needs KA_LAUNCH_EV=1 in the environment when the
   context is created); returns the number of values written (<= cap), -1 on error. */
int ka_tree_launch_ms(ka_ctx* ctx, float* ms, int cap);

/*
 * Anchor consistency = the reference's default mode (anchor_consistency_build, anchor_consistency.c:194-275,
 * called from kalign_run_seeded, aln_wrap.c:207-214).  Call between ka_tree_upload and ka_tree_run:
 * selects n_anchors anchors from seq_distances, aligns every sequence to every anchor on the device, keeps
 * the position maps in HBM; from then on every DP of ka_tree_run adds the consistency bonus that do_align
 * builds with anchor_consistency_get_bonus_profile (aln_run.c:262-295).  Like the reference it declines
 * silently (returns OK, no table) when n_anchors <= 0, numseq < 3 or there are no seq_distances.
 * n_anchors <= KA_CONS_MAX_ANCHORS (the reference's default is 5, src/parameters.c:72-73; weight 2.0).  Any number of sequences per
 * alignment: the member votes of a node count in 16 bits below 65536 members and in 32 bits from there on.
 * In a forest job every alignment gets its own table (its own anchors among its own sequences).
 * ka_tree_upload drops the table again.
 */
#define KA_CONS_MAX_ANCHORS 128 /* anchors ka_tree_build_consistency takes: up to 5 on the kernels every default-mode job uses (a DP row carries that many bonus
                                   entries + the wrap-around one in registers), 6..128 on a second set that walks a row's entries, sorted by column, along
                                   with the row's columns (`--consistency K`; round 4 stopped at 10, round 5 at 32; the reference, anchor_consistency.c:200-275,
                                   has no cap but the number of sequences) */
int ka_tree_build_consistency(ka_ctx* ctx, int n_anchors, float weight);
/* The N x K batch sharded over `nparts` GPUs: every rank uploads the same job and calls this with its
 * own `part`; it selects the same anchors, aligns only its contiguous share of the sequences (balanced by length) and
 * fills their position maps.  The table is complete once every rank's share has been copied into every other rank's
 * table: ka_tree_consistency_maps_dev gives the table in HBM (total_ints int32), ka_tree_consistency_part_range the
 * int range [lo, hi) part `part` fills -- kalign_amd/dist.py broadcasts each range in place with RCCL. */
int ka_tree_build_consistency_part(ka_ctx* ctx, int n_anchors, float weight, int part, int nparts);
int ka_tree_consistency_part_range(ka_ctx* ctx, int part, int nparts, long long* lo, long long* hi);
int ka_tree_consistency_maps_dev(ka_ctx* ctx, void** maps_dev, long long* total_ints);
/* Returns K (0: no table).  anchor_ids[K] (a forest job: K per alignment that has a table, in order of the
   alignments' first sequences); maps_out: all position maps concatenated in (i*K + k) order,
   each lens[i] ints (pos_maps, anchor_consistency.h:17-24).  Either pointer may be NULL. */
int ka_tree_get_consistency(ka_ctx* ctx, int* anchor_ids, int* maps_out);

/*
 * npairs independent seq-seq alignments (pair k = sequences ia[k], ib[k]) with unscaled
 * parameters, rows = the shorter sequence with `len_i <= len_j` deciding the swap
 * (anchor_consistency.c:44-61).  paths_out receives the coded path of pair k at poff[k]
 * (room for lens[ia]+lens[ib]+3 ints each); scores_out (optional) the top-level score.
 */
int ka_pairwise_batch(ka_ctx* ctx, const uint8_t* codes, const int* off, const int* lens, int numseq,
                      const int* ia, const int* ib, int npairs,
                      const float* subm, float gpo, float gpe, float tgpe,
                      int* paths_out, const long long* poff, float* scores_out);

/*
 * Distance estimation for the guide tree: for every pair (ia[k], ib[k]) the value of
 * calc_distance() -> bpm_block() (lib/src/sequence_distance.c:150-162, lib/src/bpm.c:356-582): block-wise Myers
 * bit-vector edit distance of the shorter sequence against the longer one, integer-exact, at most 1024 pattern
 * positions.  Sequence codes must be < 13 (the reduced alphabet kalign_run converts to before tree building,
 * aln_wrap.c:155-160, or nucleotides).  d_estimation's length term is left to the caller:
 * dm = dist + min(10000, (len_a + len_b) / 2) / 10000 (sequence_distance.c:66-69,118-120).
 */
int ka_bpm_batch(ka_ctx* ctx, const uint8_t* codes, const int* off, const int* lens, int numseq,
                 const int* ia, const int* ib, int npairs, int* dist_out);

/*
 * Realignment (kalign_run_realign, lib/src/aln_wrap.c:449-495; the member runs of `--precise`): a new guide tree from
 * a finished alignment.  compute_aln_pairwise_dist (lib/src/aln_apair_dist.c:9-86: 1 - identity over the columns
 * where both rows have a residue, all N(N-1)/2 pairs) and build_tree_from_pairwise (bisectingKmeans.c:1150-1200:
 * mean distance per sequence, then UPGMA on the N x N matrix, :974-1053) both run on the device; labels and tasks as
 * create_tasks makes them.
 *   rows             numseq rows of alnlen bytes, row_stride apart, gap_char where the reference has '-'; or NULL:
 *                    the rows the last ka_tree_aligned_rows built, still in HBM (numseq must match; row_stride,
 *                    alnlen, gap_char are ignored)
 *   tasks_abc[3*(numseq-1)], seq_distances[numseq] (may be NULL)  as for ka_guide_tree
 *   dm_out[numseq*numseq]  (may be NULL) the identity distances, before UPGMA consumed them
 * One family is a batch of one: the work is ka_aln_guide_forest's (below), with n_fam = 1.
 */
int ka_aln_guide_tree(ka_ctx* ctx, int numseq, const uint8_t* rows, long long row_stride, int alnlen, uint8_t gap_char,
                      int* tasks_abc, float* seq_distances, float* dm_out);

/*
 * kalign_run_seeded / kalign_run_realign (lib/src/aln_wrap.c:144-251, :361-527) from "sequences encoded" to "rows
 * finalised" in one call -- ka_guide_tree, ka_tree_upload, ka_tree_build_consistency, ka_tree_run, and per realignment
 * iteration rows (kept in HBM) -> ka_aln_guide_tree -> upload with KA_FLAG_KEEP_CONSISTENCY -> run; finally the rows.
 * Sequences in the order msa_sort_len_name left them.
 *   tree_codes / codes / letters   the sequences three times, all laid out by off[] / lens[]: in the alphabet of the
 *                    guide tree (reduced protein alphabet / nucleotides), in the alignment alphabet, and as printed
 *   subm, scal       as for ka_tree_upload; n_anchors 0: the reference's --fast; dm_scale NULL or the noisy tree's
 *                    multipliers (ka_guide_tree); realign_iterations 0: kalign_run_seeded
 *   rows_out[numseq * row_stride], alnlen_out[numseq]   as for ka_tree_aligned_rows; rows_out NULL leaves the alignment
 *                    on the device (alnlen_out says how long); a row_stride that turns out too small returns
 *                    KA_ERR_ROWS_STRIDE with alnlen_out filled -- ka_tree_aligned_rows then fetches the rows
 */
int ka_run_encoded(ka_ctx* ctx, int numseq, const uint8_t* tree_codes, const uint8_t* codes, const uint8_t* letters,
                   const int* off, const int* lens, const float* subm, const float* scal,
                   int n_anchors, float weight, int realign_iterations, const float* dm_scale, int n_threads,
                   uint8_t gap_char, uint8_t* rows_out, long long row_stride, int* alnlen_out);
/* The same with refinement (kalign_run_seeded / kalign_run_realign's `refine` argument): refine_mode 0 none, 1 / 2
   (optionally | KA_REFINE_ADAPTIVE) refine_alignment after the last alignment (aln_wrap.c:229-232, :506-509), 3
   KALIGN_REFINE_INLINE: every alignment of the run is create_msa_tree_inline_refine (:222-226, :498-502). */
int ka_run_encoded_refine(ka_ctx* ctx, int numseq, const uint8_t* tree_codes, const uint8_t* codes, const uint8_t* letters,
                   const int* off, const int* lens, const float* subm, const float* scal,
                   int n_anchors, float weight, int realign_iterations, const float* dm_scale, int n_threads, int refine_mode,
                   uint8_t gap_char, uint8_t* rows_out, long long row_stride, int* alnlen_out);

/*
 * Guide tree: build_tree_kmeans (lib/src/bisectingKmeans.c:177-271) -- anchors by length
 * (pick_anchor.c:34-70), N x 32 distances to the anchors, bisecting 2-means on that matrix (split2, :766-971) down
 * to clusters of fewer than 50 sequences, UPGMA on all-pairs distances inside each cluster (:974-1053), post-order
 * node labels.  The two distance batches run on the device (ka_bpm_batch); the clustering between them runs on the
 * host in the reference's fp32 evaluation order, so the task list is the reference's task list.
 *   codes            the sequences in the alphabet the reference builds its tree in: reduced protein alphabet
 *                    (ALPHA_redPROTEIN, aln_wrap.c:155-160) or nucleotides; sorted as msa_sort_len_name left them
 *   n_threads        host threads for the independent halves of the bisection (the result does not depend on it)
 *   dm_scale[numseq * min(32, numseq)]  NULL, or build_tree_kmeans_noisy (:76-175, the trees of ensemble members):
 *                    the multiplier of every anchor distance, row-major [sequence][anchor] -- what the reference
 *                    draws as max(0.1, tl_random_gaussian(rng, 1.0, sigma)) cast to float, in that order (:103-115).
 *                    The random numbers stay the caller's: they come from the reference's own generator.
 *   tasks_abc[3*(numseq-1)]  (a, b, c) in TASK_ORDER_TREE order -- what ka_tree_upload / ka_msa_tree take
 *   seq_distances[numseq]    msa->seq_distances (:244-255); may be NULL
 */
int ka_guide_tree(ka_ctx* ctx, int numseq, const uint8_t* codes, const int* off, const int* lens,
                  int n_threads, const float* dm_scale, int* tasks_abc, float* seq_distances);
/* The same with the caller's distance source: dist() must fill dist_out[k] with calc_distance(seq ia[k], seq ib[k])
 * (sequence_distance.c:150-162) for k < npairs and return 0; it is called twice (anchor batch, cluster batch).
 * Host only: needs no context and no GPU. */
typedef int (*ka_dist_fn)(void* user, int npairs, const int* ia, const int* ib, int* dist_out);
int ka_guide_tree_from(int numseq, const int* lens, ka_dist_fn dist, void* user, int n_threads,
                       const float* dm_scale, int* tasks_abc, float* seq_distances);

/*
 * The guide trees of a BATCH OF FAMILIES (a forest job, see ka_msa_tree): sequences fam_first[f] .. fam_first[f + 1] - 1 are
 * family f, n_fam families, fam_first[n_fam] = numseq sequences in all.  The three phases of build_tree_kmeans -- anchors and
 * the anchor distances; bisection and the in-cluster distances; UPGMA, tasks and seq_distances -- each run over all families
 * before the next starts: dist() is called at most twice however many families there are, with global sequence indices, both
 * members of a pair always of one family.  The families' host work runs on n_threads threads; nothing depends on their number.
 *   tasks_abc[3 * (numseq - n_fam)]  one forest task list: leaves carry their global index, internal nodes are numseq + the
 *                    task's index in this list; families in order, each family's tasks in its own TASK_ORDER_TREE order
 *   n_tasks_out      (may be NULL) the number of tasks; a family of one sequence has none, and seq_distances 0
 *   dm_scale         NULL, or the families' multiplier blocks one after the other, n_f * min(32, n_f) each
 * Per family, tasks and seq_distances are bit for bit what ka_guide_tree_from gives that family alone.  Errors name their
 * cause: "fam_first does not ascend from 0 to numseq", "empty family", "zero-length sequence".
 * ka_guide_forest_from is host only (no context, no GPU); ka_guide_forest runs the two batches on the device (ka_bpm_batch).
 */
int ka_guide_forest_from(int n_fam, const int* fam_first, const int* lens, ka_dist_fn dist, void* user, int n_threads,
                         const float* dm_scale, int* tasks_abc, int* n_tasks_out, float* seq_distances);
int ka_guide_forest(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* codes, const int* off, const int* lens,
                    int n_threads, const float* dm_scale, int* tasks_abc, int* n_tasks_out, float* seq_distances);

/*
 * The realignment trees of a batch of families (ka_aln_guide_tree: a batch of one): the identity distances of all families
 * in one launch, their row means in one, and the UPGMAs one workgroup per family (a launch per size class of the
 * one-workgroup kernel; a family of more than 6144 sequences goes through the per-merge launches on its own).  Per family,
 * tasks, seq_distances and distances depend on that family's rows alone.
 *   rows             numseq rows, row_stride apart; family f's alignment is the first alnlens[f] <= row_stride bytes of its rows
 *                    (what lies beyond is not read); or NULL: the rows the last ka_tree_aligned_rows of a forest job (or of a
 *                    single tree) left in HBM -- fam_first must describe that job's alignments; row_stride, alnlens and gap_char
 *                    are ignored
 *   tasks_abc, seq_distances (may be NULL)  as for ka_guide_forest
 *   dm_out           (may be NULL) the families' n_f x n_f matrices one after the other
 */
int ka_aln_guide_forest(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* rows, long long row_stride,
                        const int* alnlens, uint8_t gap_char, int* tasks_abc, float* seq_distances, float* dm_out);

/*
 * ka_run_encoded_refine for a batch of families in one call: the guide trees of all families (ka_guide_forest), one forest
 * ka_tree_upload with KA_FLAG_DEVICE_GAPS, ka_tree_build_consistency, ka_tree_run (refine_mode 3: ka_tree_refine), per
 * realignment iteration rows in HBM -> ka_aln_guide_forest -> upload with KA_FLAG_KEEP_CONSISTENCY -> run, refine_mode 1 / 2 (|
 * KA_REFINE_ADAPTIVE) through ka_tree_refine_trees, rows.  refine_mode 2 (KALIGN_REFINE_CONFIDENT) takes its threshold, the
 * median confidence of one alignment's edges, per tree of the forest job: per family (a family of two sequences has one
 * edge, which is refined).  All families share subm / scal.  Every
 * family comes out as ka_run_encoded_refine aligns it alone (both calls run the same sequence of steps on a forest job,
 * ka_run_encoded_refine on a job of one family): a family of n_f >= 3 sequences gets K_f = min(n_anchors, n_f) anchors, a
 * smaller one no table.  One forest job holds one anchor count, so families of equal K_f are one job and the jobs run one
 * after the other on the context.
 *   tree_codes / codes / letters, off, lens   all numseq = fam_first[n_fam] sequences, as for ka_run_encoded
 *   dm_scale         as for ka_guide_forest
 *   alnlen_out[numseq]  (may be NULL) the alignment length of every sequence's family (a family of one: its length)
 * The finished rows stay in memory the context owns until the next ka_run_encoded_batch replaces them:
 *   ka_batch_rows_size   bytes ka_batch_rows needs (-1: no finished batch)
 *   ka_batch_rows        the rows, packed: families in order, the rows of family f alnlen_f + 1 bytes apart, each ending in a
 *                        0 byte (a family of one sequence: its letters).  Fails, and loses nothing, when cap_bytes is too small.
 *   ka_batch_stats       measurements of the last batch: out6 = device ms of the guide trees' distance batches, of the
 *                        alignment runs (refinement included), of the realignment distances + UPGMA, of building rows; forest
 *                        jobs run; wall ms of the call
 *   ka_batch_refine_stats  what refine_mode 2 did in the last batch, per family in input order: thr_out[n_fam] the family's
 *                        threshold (0 for a family of one sequence), edges_out[n_fam] its tasks, refined_out[n_fam] the tasks
 *                        at or below the threshold.  Fails, naming the cause, without a finished batch, after a batch of
 *                        another refine_mode, and when n_fam is not the last batch's.
 */
int ka_run_encoded_batch(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* tree_codes, const uint8_t* codes,
                         const uint8_t* letters, const int* off, const int* lens, const float* subm, const float* scal,
                         int n_anchors, float weight, int realign_iterations, const float* dm_scale, int n_threads,
                         int refine_mode, uint8_t gap_char, int* alnlen_out);
long long ka_batch_rows_size(ka_ctx* ctx);
int ka_batch_rows(ka_ctx* ctx, uint8_t* rows_out, long long cap_bytes);
int ka_batch_stats(ka_ctx* ctx, double* out6);
int ka_batch_refine_stats(ka_ctx* ctx, int n_fam, float* thr_out, int* edges_out, int* refined_out);

/* Kernel time (HIP events on the launch stream) of the last ka_pairwise_batch / ka_bpm_batch, milliseconds. */
float ka_pairwise_kernel_ms(ka_ctx* ctx);


/*
 * ONE alignment over the GPUs of a node, driven from C (the reference's unit of parallelism is the
 * independent subtree, lib/src/aln_run.c:95-109): one process per GPU, RCCL (ncclBroadcast / ncclSend / ncclRecv /
 * ncclAllReduce over xGMI), loaded at run time -- the single-GPU library has no link-time dependency on it.
 *   ka_dist_unique_id   rank 0: the 128-byte ncclUniqueId; the launcher hands it to every rank (file, MPI, torch ...).
 *   ka_dist_create      the communicator of this rank's context (ncclCommInitRank).  world == 1 and id == NULL: none.
 *   ka_dist_plan        once per uploaded job (every rank uploads the same job): the tree is cut into one subtree per
 *                       rank, balanced by estimated DP cells; the hand-overs above the cut; this rank's subtrees planned
 *                       as one run (ka_tree_plan_tasks).  ka_dist_plan_subtrees is the pure planning function.
 *   ka_dist_consistency anchor_consistency_build sharded: this rank's share of the N x K batch, every share broadcast
 *                       in place, HBM to HBM; fails on every rank alike when one part cannot be built.
 *   ka_dist_tree_run    one step: subtrees, the merges above the cut (profiles -- and in default mode the residue ->
 *                       column tables, packed on the device -- move device to device), then every rank holds every
 *                       record and coded path (one all-reduce each over disjoint ranges).
 *   ka_dist_download    records in task order (path_off into paths) and the coded paths, identical on every rank and for
 *                       every world size.
 */
typedef struct ka_dist ka_dist;
int ka_dist_unique_id(void* id128);
int ka_dist_create(ka_ctx* ctx, int rank, int world, const void* id128, ka_dist** out);
void ka_dist_destroy(ka_dist* d);
int ka_dist_plan_subtrees(int numseq, const int* lens, int n_tasks, const int* tasks_abc, int world, int* run_rank, int* top, int* n_top);
int ka_dist_plan(ka_dist* d);
int ka_dist_get_plan(ka_dist* d, int* run_rank, int* top, int* n_top, int* n_moves);
int ka_dist_consistency(ka_dist* d, int n_anchors, float weight);
int ka_dist_tree_run(ka_dist* d);
long long ka_dist_paths_size(ka_dist* d);
int ka_dist_download(ka_dist* d, ka_task_rec* recs, int* paths, long long paths_cap, long long* used);
double ka_dist_last_ms(ka_dist* d);
/* Steps ka_dist_tree_run repeated because a device arena overflowed on SOME rank: the ranks agree on the outcome of their parts
   (all-reduce of a status word) before the gather's collectives, the ranks that overflowed grow their arenas and every rank
   runs the step again -- no rank fails, or waits in a collective, alone. */
int ka_dist_retries(ka_dist* d);
/* Tests: the ranks as threads of ONE process, each with its own context on the same GPU (RCCL refuses two ranks on one
   device): an in-process stand-in for the communicator with the same call sequence, host-synchronous. */
void* ka_dist_loopback_new(int world);
void ka_dist_loopback_free(void* loopback);
int ka_dist_create_loopback(ka_ctx* ctx, int rank, int world, void* loopback, ka_dist** out);


/* ---- the GPUs of one node under ONE caller (ka_multi.cpp) ----------------------------------------------------------------
 * ka_dist_* wants one caller per rank; a single-process C program (kalign_run behind the drop-in glue) has
 * one.  ka_multi_* runs the ranks as threads of the caller, one context + one ka_dist per device, behind calls shaped like
 * ka_tree_build_consistency / ka_tree_upload + run + download; results are the single-GPU results bit for bit
 * (lib/src/aln_run.c:95-109).  devices == NULL: devices 0 .. world-1; loopback != 0: every rank on ONE device over the
 * in-process transport (tests on one-GPU boxes).  Errors: ka_multi_last_error().
 *   ka_multi_consistency  anchor_consistency_build (anchor_consistency.c:200-275) sharded; returns the number of anchors (0: the
 *                         job declines, like the reference), < 0 on error; anchor_ids_out / maps_out as ka_tree_get_consistency
 *   ka_multi_tree_run     create_msa_tree (aln_run.c:43-78): ka_tree_upload's arguments; n_anchors > 0 = default mode (the table
 *                         is built unless flags carry KA_FLAG_KEEP_CONSISTENCY and ka_multi_consistency left it on the ranks)
 *   ka_multi_download     rank 0's records and coded paths, gaps woven on the host (gaps_out may be NULL)
 */
/* build_tree_kmeans' 2-means bisection (bisectingKmeans.c:273-402, split2 :766-971) runs on the device inside ka_guide_tree from
   2048 sequences up (ka_kmeans.hip: all of a set's up to 40 seeds side by side, every set of a recursion level in one launch,
   the order-dependent fp32 sums as chains in the reference's sample order -- the same tree, bit for bit); KA_KMEANS=0 / 1 in
   the environment forces the host / the device.  Wall time of the bisection inside the last ka_guide_tree of this process and
   where it ran (measurements). */
double ka_guide_last_bisect_ms(int* on_device);

typedef struct ka_multi ka_multi;
int ka_device_count(void);                       /* visible GPUs (hipGetDeviceCount; 0 when there is none or no driver) */
int ka_multi_create(int world, const int* devices, int loopback, ka_multi** out);
void ka_multi_destroy(ka_multi* m);
int ka_multi_world(ka_multi* m);
long long ka_multi_runs(ka_multi* m);
const char* ka_multi_last_error(void);
int ka_multi_consistency(ka_multi* m, int numseq, const uint8_t* codes, const int* off, const int* lens, const float* seq_distances,
                         int n_tasks, const int* tasks_abc, const float* subm, const float* scal, int flags,
                         int n_anchors, float weight, int* anchor_ids_out, int* maps_out);
int ka_multi_tree_run(ka_multi* m, int numseq, const uint8_t* codes, const int* off, const int* lens, const float* seq_distances,
                      int n_tasks, const int* tasks_abc, const float* subm, const float* scal, int flags,
                      int n_anchors, float weight);
long long ka_multi_paths_size(ka_multi* m);
int ka_multi_download(ka_multi* m, int numseq, const int* lens, int n_tasks, ka_task_rec* recs, int* paths_out, long long paths_cap, int* gaps_out);
/* rank r's single-GPU context (borrowed: ka_multi_destroy frees it); ka_multi_adopt: rank 0's context takes the alignment of the
 * last sharded run over (recs / gaps as ka_multi_download returned them), see ka_tree_adopt_alignment */
ka_ctx* ka_multi_ctx(ka_multi* m, int rank);
int ka_multi_adopt(ka_multi* m, const ka_task_rec* recs, const int* gaps);

/* ---- the ensemble consensus stage (ka_ens.hip, ka_ens.cpp) --------------------------------------------------------------
 * kalign_ensemble's tail (lib/src/ensemble.c:341-): scores of alignments against the members' residue pairs, the consensus
 * alignment, per-residue and per-column confidence -- without the reference's POAR table.  The support of a residue pair
 * (residue ri of sequence i, residue rj of sequence j) is the number of members that put them in one column; everything below is
 * an integer count of it, computed on the device.  Sequences are in the order of the members' rows (input / rank order).
 * A residue is an ASCII letter (isalpha in the C locale), every other byte a gap.
 *   ka_ens_create       numseq sequences of lens[s] residues, n_runs members (1..32: one bit per member in the reference's table).
 *                       The handle runs on ctx's device and stream: destroy it before ctx.
 *                       Fails for a sequence of more than 4096 residues: the reference packs a pair as ri << 20 | rj in 32 bits,
 *                       which aliases from residue index 4096 on, so its result there is not a defined contract.
 *   ka_ens_add_member   member k's rows: numseq rows of alnlen bytes, row_stride apart.  Fails when alnlen does not fit the stride
 *                       or a row's letter count differs from lens[s], or when numseq * alnlen exceeds 2^31 - 1 (also for the
 *                       alignments of ka_ens_score_rows and ka_ens_confidence).  Every member must be added before the calls below.
 *   ka_ens_score_rows   score_alignment_poar (consensus_msa.c:694-740) of any alignment of the sequences: sum_out = the exact sum
 *                       over its residue pairs of (support - 1) (-1 for a pair no member has), score_out = sum / max(n_runs - 1, 1).
 *                       The reference adds the terms one by one in double: equal within rounding, equal for equal pair sets.
 *   ka_ens_consensus    build_consensus (consensus_msa.c:372-562) at min_support >= 1 (kalign_ensemble's automatic value is
 *                       max(2, (n_runs + 2) / 3)); letters: the sequences' letters concatenated (sum of lens bytes), placed in
 *                       the consensus columns.  KA_ERR_ROWS_STRIDE with alnlen_out filled when rows_out is NULL or row_stride <
 *                       alnlen; asking again with the same arguments returns the kept result.
 *   ka_ens_confidence   compute_residue_confidence (consensus_msa.c:564-692) of an alignment: res_conf_out[numseq][alnlen]
 *                       (0 at gaps), col_conf_out[alnlen]; bit-identical to the reference.
 *   ka_ens_stats        measurements of the last calls: stats_out[10] = device ms of the position maps, of the last score, of the
 *                       consensus' count passes and write passes, host ms of the greedy and of the column order + fill, device ms of
 *                       the last confidence, host ms spent waiting for candidates, number of candidate chunks, breadth-first
 *                       searches that hit the 4096-set queue limit; level_counts_out[33] / level_ms_out[33]: candidates per support
 *                       level of the last consensus, and the device ms spent on that level alone: its write passes, plus its count
 *                       pass on a handle opened from a table, which counts level by level.  (A handle with members counts all
 *                       levels of a block of rows in one pass: that time is in stats_out[2] only.)
 */
typedef struct ka_ens ka_ens;
int  ka_ens_create(ka_ctx* ctx, int numseq, const int* lens, int n_runs, ka_ens** out);
void ka_ens_destroy(ka_ens* e);
int  ka_ens_add_member(ka_ens* e, int k, const uint8_t* rows, long long row_stride, int alnlen);
int  ka_ens_score_rows(ka_ens* e, const uint8_t* rows, long long row_stride, int alnlen, long long* sum_out, double* score_out);
int  ka_ens_consensus(ka_ens* e, int min_support, const uint8_t* letters, uint8_t* rows_out, long long row_stride, int* alnlen_out);
int  ka_ens_confidence(ka_ens* e, const uint8_t* rows, long long row_stride, int alnlen, float* res_conf_out, float* col_conf_out);
int  ka_ens_stats(ka_ens* e, double* stats_out, long long* level_counts_out, double* level_ms_out);

/* ---- the ensemble's POAR table as a file (ka_poar.hip, ka_poar.cpp, ka_ens.cpp) ------------------------------------------------
 * kalign_ensemble's save_poar_path and kalign_consensus_from_poar (lib/src/ensemble.c:349-355, 500-543): the table of pairs of
 * aligned residues the members hold, written and read as poar_table_write / poar_table_read do (lib/src/poar.c:203-325), byte for
 * byte.  All words are 32-bit little endian:
 *     "POAR" (0x524F4150) | version = 1 | numseq | n_alignments
 *     for every pair i < j (i ascending, then j):  n_entries | n_entries x { key = ri << 20 | rj ; mask (bit k: member k aligns
 *     residue ri of i with residue rj of j) }, keys ascending
 * The stage itself never needs the table (support comes from the members' position maps); it is built when asked for.
 *   ka_ens_table_size        the file's size in bytes and its number of entries, on a handle with every member added or on a handle
 *                            opened from a table.
 *   ka_ens_table_write       the file at `path`; ka_ens_table_image: the same bytes at out (cap >= the size, else an error).
 *                            A handle opened from a table gives back what it read.
 *   ka_ens_open_table        a handle whose support comes from a file (ka_ens_open_table_image: from the file's bytes in memory)
 *                            instead of members: n_runs is the file's n_alignments; ka_ens_score_rows, ka_ens_consensus,
 *                            ka_ens_confidence and ka_ens_stats work as on a handle with members, ka_ens_add_member fails.
 *                            The table is kept on the device (first entry of every pair, entries).
 *   ka_ens_n_runs            members of the handle (the file's n_alignments for an opened table).
 *   ka_ens_table_stats       out6 = device ms of the last table's count passes and of its write passes, host ms spent writing /
 *                            copying it out (ka_ens_table_write / _image) or reading and checking it (ka_ens_open_table*), entries,
 *                            chunks the table left the device in, host ms spent waiting for them.  ka_ens_stats is unchanged.
 *   ka_poar_check_image      the reader's checks alone, on the host: needs no context and no GPU.  Stricter than the reference,
 *                            which trusts the file.  Errors (ka_last_error names the cause): wrong magic; version other than 1;
 *                            numseq different from the caller's; n_alignments outside 1..32; fewer or more bytes than the counts
 *                            imply; a key with ri >= lens[i] or rj >= lens[j]; keys of a pair not strictly ascending; a mask that is
 *                            0 or has a bit at or above n_alignments.  n_runs_out / entries_out (optional) on success.
 * Two operations make new tables from tables, on the device (poar_merge / poar_select, ka_poar.hip).  An operand is a handle
 * opened from a table or a handle with every member added (its table is then built in device memory in full first; when that
 * allocation fails the error says so); operands are not modified and stay usable whether the call succeeds or not.  *out is a new
 * handle like one from ka_ens_open_table_image -- everything above works on it, ka_ens_add_member fails -- and is untouched on
 * failure.  On it ka_ens_table_stats gives the device ms of the operation's count and write passes in [0] and [1] and its
 * entries in [3].
 *   ka_ens_merge             the union of two tables of the same sequences (same context, numseq and lens): a's members keep their
 *                            bits, b's member k becomes member n_runs(a) + k; n_runs = n_runs(a) + n_runs(b) <= 32.  The table of
 *                            members 0..s-1 merged with the table of members s..R-1 is, byte for byte, the table of all R members.
 *   ka_ens_select            the table of members[0..n) of e, in that order (distinct indices below n_runs(e), 1 <= n <= n_runs(e)):
 *                            new member t is old member members[t]; an entry none of them holds is dropped.
 */
int  ka_ens_table_size(ka_ens* e, long long* bytes_out, long long* entries_out);
int  ka_ens_table_write(ka_ens* e, const char* path);
int  ka_ens_table_image(ka_ens* e, uint8_t* out, long long cap);
int  ka_ens_open_table(ka_ctx* ctx, int numseq, const int* lens, const char* path, ka_ens** out);
int  ka_ens_open_table_image(ka_ctx* ctx, int numseq, const int* lens, const uint8_t* image, long long n_bytes, ka_ens** out);
int  ka_ens_n_runs(ka_ens* e);
int  ka_ens_table_stats(ka_ens* e, double* out6);
int  ka_poar_check_image(const uint8_t* image, long long n_bytes, int numseq, const int* lens, int* n_runs_out, long long* entries_out);
int  ka_ens_merge(ka_ens* a, ka_ens* b, ka_ens** out);
int  ka_ens_select(ka_ens* e, const int* members, int n, ka_ens** out);

/* ---- scoring an alignment against a reference alignment (ka_cmp.hip, ka_cmp.cpp) -------------------------------------------
 * kalign_msa_compare, kalign_msa_compare_detailed and kalign_msa_compare_with_mask (lib/src/msa_cmp.c) on the device.  Both
 * alignments hold the same numseq sequences in the same row order (the reference pairs its rows after sorting both by name;
 * the caller does that).  A residue is an ASCII letter (isalpha in the C locale), every other byte a gap.  Every count is
 * exact and every double comes from the reference's expression: the results are bit-identical.
 *   ka_cmp_create        the reference alignment: numseq >= 2 rows of alnlen bytes, row_stride apart, row s with lens[s] letters
 *                        (at most 32767).  Builds its position maps once.  Runs on ctx's device and stream: destroy it before ctx.
 *   ka_cmp_set_mask      the scored columns of the detailed counts: with mask NULL every column when max_gap_frac < 0, else a
 *                        column whose (float)gaps / (float)numseq <= max_gap_frac (kalign_msa_compare_detailed); with a mask
 *                        (n_cols must equal the reference's alnlen) the columns where it is non-zero (kalign_msa_compare_with_mask).
 *                        Until it is called, every column is scored.
 *   ka_cmp_score         one test alignment.  Fails when the width does not fit the stride or a row's letter count differs
 *                        from lens[s].  counts_out[12] (optional): struct cmp_stats' six counts (ref_total_aligned_pairs,
 *                        ref_total_gap_pairs, identical_aligned, identical_gaps, test_total_aligned_pairs, test_total_gap_pairs),
 *                        the four detailed counts (ref_scored_pairs, test_pairs, common_scored, common_all), tc_correct, tc_total.
 *                        scores_out[5] (optional): recall, precision, f1, tc (struct poar_score) and the SP score in double;
 *                        sp_out (optional): the float kalign_msa_compare returns.
 *   ka_cmp_score_batch   n_tests test alignments (their own widths and strides), counts_out[n_tests * 12], scores_out[n_tests * 5],
 *                        sp_out[n_tests]: exactly what n_tests calls of ka_cmp_score return, with fewer launches.
 *   ka_cmp_stats         device ms: stats_out[4] = the reference's maps (ka_cmp_create), the test maps, the pair walk and the TC
 *                        pass of the last score call (summed over a batch).
 */
typedef struct ka_cmp ka_cmp;
int  ka_cmp_create(ka_ctx* ctx, int numseq, const int* lens, const uint8_t* ref_rows, long long row_stride, int alnlen, ka_cmp** out);
void ka_cmp_destroy(ka_cmp* h);
int  ka_cmp_set_mask(ka_cmp* h, float max_gap_frac, const int* mask, int n_cols);
int  ka_cmp_score(ka_cmp* h, const uint8_t* test_rows, long long row_stride, int alnlen, long long* counts_out, double* scores_out, float* sp_out);
int  ka_cmp_score_batch(ka_cmp* h, int n_tests, const uint8_t* const* test_rows, const long long* row_strides, const int* alnlens,
                        long long* counts_out, double* scores_out, float* sp_out);
int  ka_cmp_stats(ka_cmp* h, double* stats_out);

/* ---- scoring a batch of families, each against its own reference alignment (ka_cmp.hip, ka_cmp.cpp, ka_cmp_fam.cpp) --------
 * What ka_cmp_create + ka_cmp_set_mask + ka_cmp_score return for every family alone -- twelve counts, five doubles and the
 * float SP score, bit for bit -- for all families of a batch in a number of launches that does not grow with the batch,
 * with one copy back and one synchronisation per score call.  The references stay on the device: the loop of a benchmark
 * (one reference per family, new test alignments per parameter set) creates once and scores many times.
 *   Families   fam_first[n_fam + 1] and lens[numseq] as ka_run_encoded_batch takes them; two sequences per family at least.
 *   Rows       packed as ka_batch_rows hands them out: families in order, the rows of family f alnlens[f] + 1 bytes apart
 *              (the byte after a row is not read), so its output is test_rows as it stands.  alnlens is per family.
 *   ka_cmp_fam_check      every check of a packed batch, on the host alone (no context, no GPU): fam_first ascends from 0
 *                         ("fam_first does not ascend from 0 to numseq", "empty family"), and per family what ka_cmp_create /
 *                         ka_cmp_score check.  A message names the family and ends in the cause the one-family call gives:
 *                         "ka_cmp_fam_check: family 3: row 1 holds 7 letters, its sequence 8 (...)".
 *   ka_cmp_fam_create     the reference alignments; runs the check, then builds their position maps once.  Limits per family
 *                         as ka_cmp_create's; over the batch fewer than 2^31 residues and fewer than 2^31 reference columns.
 *                         Runs on ctx's device and stream: destroy it before ctx.
 *   ka_cmp_fam_set_masks  the column rule of every family: with mask_off[f] >= 0 the ref_alnlens[f] ints at masks + mask_off[f]
 *                         (kalign_msa_compare_with_mask), else max_gap_frac[f] (kalign_msa_compare_detailed; below 0: every
 *                         column).  max_gap_frac NULL: -1 for every family; masks or mask_off NULL: no masks.  Until it is
 *                         called, every column is scored.
 *   ka_cmp_fam_score      one test alignment per family; runs the check on them.  A refused batch launches nothing and leaves
 *                         the handle usable.  counts_out[n_fam * 12], scores_out[n_fam * 5], sp_out[n_fam] (each optional)
 *                         as ka_cmp_score lays them out.
 *   ka_cmp_fam_stats      device ms: stats_out[4] as ka_cmp_stats, each over the whole batch.
 */
typedef struct ka_cmp_fam ka_cmp_fam;
int  ka_cmp_fam_check(int n_fam, const int* fam_first, const int* lens, const uint8_t* rows, const int* alnlens);
int  ka_cmp_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const int* lens, const uint8_t* ref_rows, const int* ref_alnlens,
                       ka_cmp_fam** out);
void ka_cmp_fam_destroy(ka_cmp_fam* h);
int  ka_cmp_fam_set_masks(ka_cmp_fam* h, const float* max_gap_frac, const int* masks, const long long* mask_off);
int  ka_cmp_fam_score(ka_cmp_fam* h, const uint8_t* test_rows, const int* test_alnlens, long long* counts_out, double* scores_out,
                      float* sp_out);
int  ka_cmp_fam_stats(ka_cmp_fam* h, double* stats_out);

/* ---- where a test alignment agrees with its reference: per residue and per column (ka_cmp.hip, ka_cmp.cpp, ka_cmp_fam.cpp) ----
 * The score entries above say how good a test alignment is; these say where it is right.  They are the ground truth that the
 * confidences of the ensemble stage (ka_ens_fam_confidence) predict: per test column the verdict of _column_correctness of
 * the reference's benchmarks/downstream/calibration.py, per residue the counts behind it.
 *   Kept from the comparison stage: a residue is an ASCII letter, every other byte a gap; rows are paired by position; the
 *   checks are ka_cmp_fam_check's.  Residues are numbered flat over the handle as the stage numbers them: sequences in order,
 *   a sequence's residues in order; T is their number.  The column rule (ka_cmp_set_mask, ka_cmp_fam_set_masks) plays no
 *   part: every column is reported.
 *   For residue e = residue ri of sequence i, over the other sequences j of its family, with col[i][ri] the column of the
 *   residue and res[j][c] the residue of j at column c (or -1):
 *       pR = resR[j][colR[i][ri]]        pT = resT[j][colT[i][ri]]
 *   res_counts[3][T]   int32: plane 0 #[pR >= 0], plane 1 #[pT >= 0], plane 2 #[pR >= 0 && pR == pT] -- its aligned partners
 *                      in the reference, in the test, and in both.  The planes sum to ref_total_aligned_pairs,
 *                      test_total_aligned_pairs and identical_aligned of the score call.
 *   test columns       flat over the call, families in order (the sum of the test alnlens), per column: residues int32 (k);
 *                      common int64 (plane 2 summed over the column's residues); correct uint8: 1 when k <= 1 or all k
 *                      residues lie in one column of the reference.  correct == (common == k (k - 1)).
 *   reference columns  flat over the handle (the sum of the reference alnlens): the same three with the sides swapped --
 *                      correct is TC's verdict per column: over the scored columns with k >= 2 it sums to tc_correct.
 *   ka_cmp_detail            one test alignment of a ka_cmp handle, as ka_cmp_score takes it.
 *   ka_cmp_fam_detail        one test alignment per family, as ka_cmp_fam_score takes them.  Every output is optional.  A
 *                            refused batch launches nothing and leaves the handle usable; the handle scores exactly as before
 *                            afterwards.  A call is one upload of the rows, one copy back and one host synchronisation; its
 *                            launches (the test maps, the detailed walk once per LDS class in use, the column pass) do not
 *                            depend on the number of families.
 *   ka_cmp_detail_stats, ka_cmp_fam_detail_stats   out5: device ms of the test maps, the detailed walk and the column pass,
 *                            then the kernel launches and host synchronisations of the last detail call (all 0 before the
 *                            first, and after a refused one).
 *   ka_calibration     host only (no context, no GPU): brier_score, expected_calibration_error and calibration_curve of the
 *                      same file over (predicted, actual) items.  Segment s is the items seg_first[s] .. seg_first[s + 1] - 1;
 *                      every output has n_seg + 1 slots, the last the pool of all items in order (_aggregate_summary pools
 *                      its cases so).  Per slot: brier, ece, bin_fraction[n_bins] (NaN for an empty bin), bin_counts[n_bins];
 *                      each output optional.  The reference's order of operations: serial double sums in item order,
 *                      b = (int)(p * n_bins) clamped to the last bin; an empty slot gives 0.0, 0.0, NaNs and zeros.  Refused
 *                      before anything is written, the message naming the item: n_bins < 1, seg_first not ascending from 0,
 *                      predicted outside [0, 1] or NaN (the reference would index a negative bin), actual above 1.
 */
int  ka_cmp_detail(ka_cmp* h, const uint8_t* test_rows, long long row_stride, int alnlen, int* res_counts, int* tcol_residues,
                   long long* tcol_common, uint8_t* tcol_correct, int* rcol_residues, long long* rcol_common, uint8_t* rcol_correct);
int  ka_cmp_fam_detail(ka_cmp_fam* h, const uint8_t* test_rows, const int* test_alnlens, int* res_counts, int* tcol_residues,
                       long long* tcol_common, uint8_t* tcol_correct, int* rcol_residues, long long* rcol_common, uint8_t* rcol_correct);
int  ka_cmp_detail_stats(ka_cmp* h, double* out5);
int  ka_cmp_fam_detail_stats(ka_cmp_fam* h, double* out5);
int  ka_calibration(int n_seg, const long long* seg_first, const double* predicted, const uint8_t* actual, int n_bins, double* brier,
                    double* ece, double* bin_fraction, long long* bin_counts);

/* ---- the ensemble consensus stage for a batch of families (ka_ens.hip, ka_ens_fam.cpp) ----------------------------------------
 * What ka_ens_create + ka_ens_add_member + ka_ens_score_rows + ka_ens_consensus + ka_ens_confidence return for every family
 * alone -- equal integer sums, doubles from the same expressions, byte-identical rows, bit-identical confidences -- for all
 * families of a batch with the same number of members.  The number of launches and host synchronisations of a call depends
 * on n_runs and on the number of candidate chunks, never on the number of families.  The POAR table as a file
 * (ka_ens_table_*, ka_ens_open_table*, ka_ens_merge, ka_ens_select) stays a one-family operation: use ka_ens for it.
 *   Families   fam_first[n_fam + 1] and lens[numseq] as ka_run_encoded_batch takes them.
 *   Rows       packed as ka_batch_rows hands them out: families in order, the rows of family f alnlens[f] + 1 bytes apart
 *              (the byte after a row is not read), so the output of ka_run_encoded_batch is a member as it stands.  alnlens
 *              is per family.
 *   Limits     per family those of ka_ens_create (n_runs 1..32, no sequence above 4096 residues, any numseq >= 1); over the
 *              batch fewer than 2^31 residues and fewer than 2^31 row bytes.
 *   ka_ens_fam_check          every check of a packed batch, on the host alone (no context, no GPU): fam_first ascends from 0
 *                             ("fam_first does not ascend from 0 to numseq", "empty family"), and per family what ka_ens_create
 *                             and ka_ens_add_member / ka_ens_score_rows check.  A message names the family and ends in the
 *                             cause the one-family call gives: "ka_ens_fam_check: family 3: row 1 holds 7 letters, its
 *                             sequence 8 (...)".  ka_ens_fam_add_member, _score and _confidence run it first: a refused batch
 *                             launches nothing and leaves the handle usable.
 *   ka_ens_fam_create         n_runs and the families are checked before ctx is touched.  Runs on ctx's device and stream:
 *                             destroy it before ctx.
 *   ka_ens_fam_add_member     member k (0 <= k < n_runs) of every family: one upload.  Every member must be added before the
 *                             calls below.
 *   ka_ens_fam_score_members  ka_ens_score_rows of every member of every family from the maps already on the device (nothing
 *                             is uploaded again): sums_out / scores_out [n_runs * n_fam], member k of family f at k * n_fam + f.
 *   ka_ens_fam_score          one alignment per family; alnlens[f] < 0: family f has no rows in the batch and is skipped, its
 *                             outputs are 0.  sums_out / scores_out [n_fam] (each optional).
 *   ka_ens_fam_consensus      ka_ens_consensus at min_support[f] >= 1 per family; letters: the letters of all sequences
 *                             concatenated.  All support levels are counted in one pass; the candidates leave the device
 *                             level by level, highest first, a level in chunks of whole families of at most KA_ENS_CHUNK
 *                             candidates (a larger family is a chunk of its own), double-buffered; the families of a chunk are
 *                             dealt to n_threads (1..16) host threads, each running the greedy union -- and after the last
 *                             chunk the column order and the fill -- of whole families.  The result does not depend on
 *                             n_threads.  alnlens_out[n_fam].
 *   ka_ens_fam_rows_size / ka_ens_fam_rows   the rows of the last consensus, packed as above with a 0 byte after each row
 *                             (-1 / an error when there is none).
 *   ka_ens_fam_confidence     ka_ens_confidence of one alignment per family: res_conf_out per family [N_f][alnlens[f]] and
 *                             col_conf_out [alnlens[f]], families back to back.
 *   ka_ens_fam_stats          stats_out[21]: device ms of the position maps [0], of the last score call [1], of the last
 *                             consensus' count pass [2] and write passes [3], of the last confidence [4]; of the last consensus
 *                             host ms of the greedy union, column order and fill summed over the threads [5] and as wall time
 *                             [6], host ms waiting for candidates [7], chunks [8], candidates [9], breadth-first searches that
 *                             hit the 4096-set queue limit [10]; then kernel launches and host synchronisations of the last
 *                             add_member [11, 12], score_members [13, 14], score [15, 16], consensus [17, 18] and confidence
 *                             [19, 20] (the members' maps count for the call that builds them).
 * One host-only seam for tests, needing no context and no GPU:
 *   ka_debug_ens_fam_consensus_host   the greedy union, the column order and the fill over given candidate lists with the thread
 *                             dealing of ka_ens_fam_consensus: cand holds two ints per candidate (residue numbers flat inside
 *                             the family), family f's candidates from cand_first[f] to cand_first[f + 1], in the order they
 *                             are to be replayed.  alnlens_out[n_fam] is always filled; KA_ERR_ROWS_STRIDE when rows_out is
 *                             NULL or cap is below the packed size.
 */
typedef struct ka_ens_fam ka_ens_fam;
int  ka_ens_fam_check(int n_fam, const int* fam_first, const int* lens, const uint8_t* rows, const int* alnlens);
int  ka_ens_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const int* lens, int n_runs, ka_ens_fam** out);
void ka_ens_fam_destroy(ka_ens_fam* h);
int  ka_ens_fam_add_member(ka_ens_fam* h, int k, const uint8_t* rows, const int* alnlens);
int  ka_ens_fam_score_members(ka_ens_fam* h, long long* sums_out, double* scores_out);
int  ka_ens_fam_score(ka_ens_fam* h, const uint8_t* rows, const int* alnlens, long long* sums_out, double* scores_out);
int  ka_ens_fam_consensus(ka_ens_fam* h, const int* min_support, const uint8_t* letters, int n_threads, int* alnlens_out);
long long ka_ens_fam_rows_size(ka_ens_fam* h);
int  ka_ens_fam_rows(ka_ens_fam* h, uint8_t* out, long long cap);
int  ka_ens_fam_confidence(ka_ens_fam* h, const uint8_t* rows, const int* alnlens, float* res_conf_out, float* col_conf_out);
int  ka_ens_fam_stats(ka_ens_fam* h, double* stats_out);
int  ka_debug_ens_fam_consensus_host(int n_fam, const int* fam_first, const int* lens, const long long* cand_first, const int* cand,
                                     const uint8_t* letters, int n_threads, int* alnlens_out, uint8_t* rows_out, long long cap);

/* ---- summaries and trimming of the finished rows of a batch of families (ka_sum.hip, ka_sum.cpp) -----------------------------
 * What python-kalign's kalign.utils computes from one alignment -- alignment_stats, consensus_sequence, remove_gap_columns,
 * trim_alignment -- for all families of a batch in a number of launches that does not grow with the batch; one alignment is a
 * batch of one.  Every count is an exact integer and every double the one division named below, so the results equal the
 * utilities' bit for bit.
 *   A byte     is a gap when it equals gap_char ('-' gives the utilities' behaviour); every other byte is a character and is
 *              compared as a byte: upper and lower case differ, '.' and '*' are characters.  (Not the isalpha rule of the
 *              comparison and ensemble stages.)
 *   Families   fam_first[n_fam + 1]; a family has one row at least.  No sequence lengths are needed.
 *   Rows       packed as ka_batch_rows hands them out: families in order, the rows of family f alnlens[f] + 1 bytes apart
 *              (the byte after a row is not read).  alnlens[f] >= 1, a family holds fewer than 2^31 cells, the batch fewer
 *              than 2^31 columns and fewer than 2^31 chunks of 256 columns over its rows.
 *   Columns    are numbered flat over the batch, families in order: the sum of alnlens in all.
 *   ka_sum_fam_check     every check of a packed batch, on the host alone (no context, no GPU): "ka_sum_fam_check: fam_first
 *                        does not ascend from 0 to numseq", "ka_sum_fam_check: empty family", "ka_sum_fam_check: family 3:
 *                        alnlen 0".
 *   ka_sum_fam_create    runs the check, uploads the rows in one copy and builds the column table, the families' sums and
 *                        their character sets once.  Runs on ctx's device and stream: destroy it before ctx.
 *   ka_sum_fam_columns   per column (each output optional): gaps; distinct characters; the most frequent character and its
 *                        count -- among characters of equal highest count the one whose first occurrence is in the lowest row,
 *                        as Counter.most_common; gap_char and 0 in an all-gap column --; the sum over the column's characters a
 *                        of n_a (n_a - 1) / 2.
 *   ka_sum_fam_summary   counts_out[n_fam * 6]: gaps, cells, conserved columns (a character and one distinct), columns,
 *                        matching pairs (the sum of same_pairs), compared pairs (the sum of k (k - 1) / 2, k the characters
 *                        of a column); values_out[n_fam * 3]: gap_fraction = gaps / cells, conservation = conserved / columns,
 *                        identity = matching / compared (0 when nothing is compared), each (double)a / (double)b.  Over all
 *                        pairs of rows the matches at columns where both have a character are the matching pairs, the
 *                        positions compared the compared pairs: alignment_stats' identity without a pair walk.
 *   ka_sum_fam_consensus thresholds[n_fam] in [0, 1] (NULL: 0.5).  A column's character is gap_char when it holds no
 *                        character, top_char when (double)top_count / (double)k >= threshold, else the family's ambiguous
 *                        character: 'N' when every character of the family, upper-cased, lies in ATCGUN, else 'X'.  out: one
 *                        row per family, packed like the rows (a 0 byte after each); ambiguous_out[n_fam].  Each optional.
 *   ka_sum_fam_keep      the columns a rule keeps: with mask_off[f] >= 0 the alnlens[f] ints at masks + mask_off[f] (non-zero
 *                        keeps; masks holds the sum of alnlens ints at most: an offset that passes that end is refused), else
 *                        (double)n_gap / (double)n_f < gap_thresholds[f] (in [0, 1]; NULL: 1.0 for every family, which drops
 *                        the all-gap columns).  masks or mask_off NULL: no masks.  keep_out: 0 / 1 per column, the layout
 *                        ka_cmp_fam_set_masks takes; new_alnlens[n_fam]: kept columns.  Each optional.
 *   ka_sum_fam_compact   the rows with only the columns the same rule keeps, left on the device; then ka_sum_fam_rows_size
 *                        and ka_sum_fam_rows hand them out packed with their new widths and a 0 byte after each row (a
 *                        family that keeps nothing has rows of width 0; -1 / an error before the first compact).  The
 *                        handle's own rows are untouched: any number of rules can be tried on one upload.
 *   ka_sum_fam_stats     stats_out[6]: device ms of the column table [0] and of the last consensus [1], keep [2] and compact
 *                        [3]; kernel launches [4] and host synchronisations [5] of the last create, consensus, keep or compact
 *                        call (0 and 0 when it was refused).  The hand-outs -- columns, summary, rows -- are copies of what
 *                        those calls left and do not count.
 * A refused call (a threshold outside [0, 1] or NaN, a mask offset past the end) launches nothing and leaves the handle usable.
 *
 * The pairwise identity matrices (kalign.utils.pairwise_identity_matrix) of the rows a handle holds -- no new upload.  For
 * family f of N_f rows and every pair (i, j):
 *   compared[i][j]  the columns where both rows hold a character (the rule for a byte above, with the handle's gap_char);
 *   matches[i][j]   those of them where the two bytes are equal; on the diagonal both are the characters of row i;
 *   identity[i][j]  (double)matches / (double)compared for i != j, 0.0 when compared is 0; identity[i][i] is 1.0 always, for
 *                   an all-gap row too (the utility sets it without looking).
 * All three are symmetric and both triangles are written.  The matrices are packed, families in order: family f's N_f x N_f
 * block is row-major and starts at entry sum over g < f of N_g^2.  Counts are int32 (a width is below 2^31).
 *   ka_sum_fam_identity_entries  host only (no context, no GPU): the entries of each matrix, the sum of N_f^2; -1 with
 *                        ka_last_error "ka_sum_fam_identity_entries: fam_first does not ascend from 0 to numseq",
 *                        "ka_sum_fam_identity_entries: empty family" or, when the sum reaches 2^31,
 *                        "ka_sum_fam_identity_entries: family 0: 46341 rows bring the matrices to 2147488281 entries; a batch
 *                        holds fewer than 2^31" (the family at which the sum passes the bound, and the sum there).
 *   ka_sum_fam_identity  each output optional, ka_sum_fam_identity_entries entries long.  The first call -- or the first
 *                        after calls that computed nothing -- runs one kernel over the upper-triangle tiles of all families
 *                        and leaves the three matrices on the device; later calls are copies.  One launch and one host
 *                        synchronisation, whatever the number of families.  A batch that ka_sum_fam_identity_entries refuses
 *                        is refused here ("ka_sum_fam_identity: family ...") before anything is launched, and the handle
 *                        stays usable.
 *   ka_sum_fam_identity_stats  out3: device ms of the identity pass [0]; kernel launches [1] and host synchronisations [2] of
 *                        the call that computed the matrices (1 and 1; all 0 before).  Later calls, which only copy, leave the
 *                        three values as they are, and no identity call touches ka_sum_fam_stats' six.
 *
 * The gap structure of the rows a handle holds, and the rows without their gaps -- no new upload (ABI 26).  What the
 * reference's benchmarks/analysis.py: compute_gap_stats measures of an alignment (the gap opens per sequence of
 * vsm_ensemble_experiment.py: _alignment_stats are gap blocks / N), and what dealign_msa and the strip loop of
 * kalign_post_realign make of it.  Both come from a walk along rows, a wave per row, with the rule for a byte above and the
 * handle's gap_char; nothing at or past column W of a row is read.  Rows are numbered flat over the batch, families in order.
 *   A row's record  int32[4]: characters; leading gap columns (before its first character); trailing gap columns (after its
 *                   last); gap blocks, a block being a maximal run of gaps.  An all-gap row has leading = trailing = W and
 *                   one block: it counts its W gaps on both sides, as the reference's lstrip / rstrip arithmetic does.
 *   ka_sum_fam_gaps      each output optional.  row_recs_out[numseq * 4]: the records.  counts_out[n_fam * 8], per family:
 *                        rows N [0], columns W [1], characters [2], gaps [3], gap blocks [4], terminal [5]: the sum over rows
 *                        of leading + trailing (an all-gap row adds 2 W), internal [6]: the sum over rows of
 *                        max(0, gaps_r - leading_r - trailing_r), gappy columns [7]: those with 2 n_gap > N (the reference's
 *                        gaps_in_col > n_seqs / 2 in exact integers).  values_out[n_fam * 7]: mean_seq_length = characters /
 *                        N [0], expansion_factor = W / mean_seq_length when that mean is > 0, else 0.0 [1] (two roundings, as
 *                        the reference computes it), gap_fraction = gaps / (N W) [2], mean_gap_block_len = gaps / blocks, 0.0
 *                        without a block [3], mean_terminal_gap = terminal / N [4], mean_internal_gap = internal / N [5],
 *                        gappy_column_fraction = gappy / W [6], each (double)a / (double)b, computed on the host from the
 *                        counts and nowhere else.  The first call -- or ka_sum_fam_ungapped before it -- runs the row pass
 *                        and the gappy-column pass over the whole batch: two launches and one host synchronisation, whatever
 *                        the number of families; later calls are copies.
 *   ka_sum_fam_gap_values  host only (no context, no GPU): values_out[n_fam * 7] from counts[n_fam * 8], the expressions
 *                        above and their zero-denominator cases (N, N W, W, blocks or the mean 0: 0.0).
 *                        "ka_sum_fam_gap_values: bad arguments" for n_fam < 1 or a NULL.
 *   ka_sum_fam_ungapped_size  the characters of the batch, the bytes ka_sum_fam_ungapped writes (known from the column
 *                        table: nothing is launched); -1 with "ka_sum_fam_ungapped_size: bad arguments" for a NULL handle.
 *   ka_sum_fam_ungapped  out: every row's characters in order, packed, row after row with nothing between them;
 *                        row_off_out[numseq + 1] (optional): row r lies at out + row_off_out[r], row_off_out[numseq] is the
 *                        size.  The offsets are the running sum of the records' characters, 64 bits.  The first call runs
 *                        the row pass if no call has yet (counted as ka_sum_fam_gaps' own), then one launch and one host
 *                        synchronisation, and leaves the rows on the device; later calls are copies.  A cap below the size
 *                        is refused before anything is launched: "ka_sum_fam_ungapped: 3 bytes do not hold the ungapped
 *                        rows (5)".  A batch without a character is valid: size 0, nothing launched or waited for by the
 *                        ungap pass, out may be NULL.
 *   ka_sum_fam_gap_stats out6: device ms of the row pass and the gappy pass [0] and of the ungap pass [1]; kernel launches
 *                        [2] and host synchronisations [3] of the computation of the gaps (2 and 1), and [4], [5] of the
 *                        ungapped rows (1 and 1; 0 and 0 for a batch without a character).  All 0 before; copies leave them
 *                        as they are; these calls touch neither ka_sum_fam_stats' six values nor
 *                        ka_sum_fam_identity_stats' three.
 * A refused call launches nothing and leaves the handle usable.
 */
typedef struct ka_sum_fam ka_sum_fam;
int  ka_sum_fam_check(int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens);
int  ka_sum_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens, int gap_char, ka_sum_fam** out);
void ka_sum_fam_destroy(ka_sum_fam* h);
int  ka_sum_fam_columns(ka_sum_fam* h, int* n_gap, int* n_distinct, uint8_t* top_char, int* top_count, long long* same_pairs);
int  ka_sum_fam_summary(ka_sum_fam* h, long long* counts_out, double* values_out);
int  ka_sum_fam_consensus(ka_sum_fam* h, const double* thresholds, uint8_t* out, uint8_t* ambiguous_out);
int  ka_sum_fam_keep(ka_sum_fam* h, const double* gap_thresholds, const int* masks, const long long* mask_off, int* keep_out, int* new_alnlens);
int  ka_sum_fam_compact(ka_sum_fam* h, const double* gap_thresholds, const int* masks, const long long* mask_off, int* new_alnlens);
long long ka_sum_fam_rows_size(ka_sum_fam* h);
int  ka_sum_fam_rows(ka_sum_fam* h, uint8_t* out, long long cap);
int  ka_sum_fam_stats(ka_sum_fam* h, double* stats_out);
long long ka_sum_fam_identity_entries(int n_fam, const int* fam_first);
int  ka_sum_fam_identity(ka_sum_fam* h, int* matches_out, int* compared_out, double* identity_out);
int  ka_sum_fam_identity_stats(ka_sum_fam* h, double* out3);
int  ka_sum_fam_gaps(ka_sum_fam* h, long long* counts_out, double* values_out, int* row_recs_out);
int  ka_sum_fam_gap_values(int n_fam, const long long* counts, double* values_out);      /* host only: no context, no GPU */
long long ka_sum_fam_ungapped_size(ka_sum_fam* h);
int  ka_sum_fam_ungapped(ka_sum_fam* h, uint8_t* out, long long cap, long long* row_off_out);
int  ka_sum_fam_gap_stats(ka_sum_fam* h, double* out6);

/*
 * The input stage (ABI 28): a batch of families from raw text to the three encodings ka_run_encoded_batch takes, and from
 * there to rows in the caller's order.  What the reference does at its front door, per family:
 *   msa_io.c:454-468          "msa->letter_freq[(int)line[i]]++; if(isalpha((int)line[i])){ ... seq_ptr->seq[seq_ptr->len] =
 *                             line[i]; seq_ptr->len++; ... }else if(ispunct((int)line[i])){ seq_ptr->gaps[seq_ptr->len]++; }"
 *   msa_op.c:142-213          detect_alphabet: "DNA[i] = log(0.0001 * 1.0 / 116.0); protein[i] = log(0.0001 * 1.0 / 88.0);",
 *                             "acgtunACGTUN" at log(0.9999 * 1.0 / 12.0), "acdefghiklmnpqrstvwyACDEFGHIKLMNPQRSTVWY" at
 *                             log(0.9999 * 1.0 / 40.0); "if(msa->letter_freq[i]){ dna_prob += DNA[i] * (double)
 *                             msa->letter_freq[i]; prot_prob += protein[i]* (double) msa->letter_freq[i]; }"
 *   msa_op.c:215-271          detect_aligned: "if(gaps){ if(min_len == max_len){ msa->aligned = ALN_STATUS_ALIGNED; }else{ ...
 *                             ALN_STATUS_UNKNOWN; } }else{ if(min_len == max_len){ ... ALN_STATUS_UNKNOWN; }else{ ...
 *                             ALN_STATUS_UNALIGNED; } }" (msa_struct.h:14-17: UNALIGNED 1, ALIGNED 2, UNKNOWN 3)
 *   aln_wrap.c:146-149        "if(msa->aligned != ALN_STATUS_UNALIGNED){ RUN(dealign_msa(msa)); }"
 *   msa_sort.c:62-80          sort_by_len_name: "if((*one)->len > (*two)->len){ return -1; }else if((*one)->len ==
 *                             (*two)->len){ int c = strncmp((*one)->name, (*two)->name, MSA_NAME_LEN); if(c < 0){ return -1;
 *                             }else{ return 1; } }else{ return 1; }"
 *   msa_op.c:358-364          convert_msa_to_internal: "if(t[(int) seq->seq[j]] == -1){ WARNING_MSG(...); seq->s[j] = 0; }"
 *   msa_check.c:301-310       GCGchecksum: "chk = (chk + (i % 57 + 1) * (toupper((int) seq[i]))) % 10000;"
 *   alphabet.c:179-302, 399-430  create_protein_BZX, create_default_DNA, create_reduced_protein, clean_and_set_to_extern
 *   A byte     b < 128 is a residue when it is a letter (A-Z, a-z; kept as given, case included), a gap character when it
 *              is punctuation (33-47, 58-64, 91-96, 123-126), and is dropped otherwise (white space, digits, control bytes).
 *              A byte >= 128 is an error: the reference indexes letter_freq with it, which is undefined.  Gap characters
 *              are always discarded -- an input with one is never UNALIGNED, and everything else is dealigned -- but they
 *              are counted, for the aligned status and the histogram.
 *   Text       text holds the sequences' raw bytes; sequence i of the batch is text[seq_off[i] .. seq_off[i + 1]), seq_off
 *              [numseq + 1] ascends from 0, a sequence holds fewer than 2^31 bytes.  fam_first[n_fam + 1] as everywhere; a
 *              family has one sequence at least.  names / name_off[numseq + 1] the same way, or both NULL: no names.
 *   Histogram  freq[128] per family counts every byte handed in, punctuation and dropped bytes included.
 *   Biotype    per family, 0 protein, 1 DNA: biotype_in[f] when that is 0 or 1 (biotype_in NULL or -1: detect).  Detection
 *              is detect_alphabet on the host from the device's integer histogram: two sums in double over i = 0..127 in
 *              ascending order, zero counts skipped; > gives DNA, < protein, equality is an error for that family.
 *   Status     per family 1 unaligned, 2 aligned, 3 unknown, from residues + gap characters per sequence.  Reported only.
 *   Order      per family: more residues first; ties by strncmp of the names over 256 bytes; without names, and for equal
 *              names, by input index (the reference's comparator is inconsistent for equal names; this defines what it
 *              leaves open, and is what its library entry gets from the "s%07d" names it makes up).
 *   Codes      three tables of 128 entries: nucleotides (both planes of a DNA family), the reduced protein alphabet (tree
 *              plane of a protein family), the protein alphabet with B Z X (its alignment plane); lower case = upper case;
 *              -1 = no code.  A letter with no code becomes code 0 and is counted per family.  The two protein tables give
 *              a code to the same letters.
 *   Checksum   per sequence, GCGchecksum over the residues as kept.
 *   A sequence with no residue is an error naming family and sequence.  The reference drops such sequences
 *   (msa_check.c:82-133); a batch whose rows silently go missing is worse than a refusal.
 *
 * Host only (no context, no GPU):
 *   ka_in_tables     out3x128: nucleotides, reduced protein, protein, in this order.
 *   ka_in_detect     biotype_out from freq128, or "ka_in_detect: could not determine the alphabet".
 *   ka_in_order      order_out[numseq]: sorted position -> input index, batch-wide (family f's positions are fam_first[f] ..
 *                    fam_first[f + 1] - 1); names / name_off may be NULL.
 *   ka_in_fam_check  "ka_in_fam_check: fam_first does not ascend from 0 to numseq", "ka_in_fam_check: empty family",
 *                    "ka_in_fam_check: seq_off does not ascend from 0 to n_bytes", "ka_in_fam_check: family 0, sequence 1:
 *                    2147483648 bytes; a sequence holds fewer than 2^31".
 * The stage:
 *   ka_in_fam_create runs the check, uploads the text in one copy and launches twice: the scan (counts, checksums, first
 *                    byte >= 128, histograms), then -- after detection, status, order and offsets on the host -- the encode
 *                    (three planes in sorted order).  Two launches and two host synchronisations (the host needs the counts,
 *                    then the planes), whatever the batch.  Fails naming the cause: the check's messages, "ka_in_fam_create:
 *                    family 1, sequence 0: byte 0xc3 at offset 5" (the first offender in batch order; sequence numbers are
 *                    within the family, offsets within the sequence's raw bytes), "ka_in_fam_create: family 1, sequence 2
 *                    has no residue", "ka_in_fam_create: family 0: could not determine the alphabet".  Runs on ctx's device
 *                    and stream: destroy it before ctx.
 *   ka_in_fam_sequences  recs_out[numseq * 4] in input order: residues, gap characters, dropped bytes, checksum.
 *   ka_in_fam_families   recs_out[n_fam * 5]: biotype, aligned status, min and max residues, letters without a code;
 *                    freq_out[n_fam * 128] (may be NULL).
 *   ka_in_fam_order  order_out[numseq] as ka_in_order.
 *   ka_in_fam_size   residues of the batch (the bytes of each plane).
 *   ka_in_fam_encoded  the three planes, off[numseq] and lens[numseq] in sorted order, as ka_run_encoded_batch takes them
 *                    (each optional; refused when the batch holds 2^31 residues or more).
 *   ka_in_fam_run    aligns the families whose biotype is `biotype` with that biotype's subm / scal: their planes go to the
 *                    path ka_run_encoded_batch runs (no noisy trees), so each family comes out as ka_run_encoded_refine
 *                    aligns it alone, and their rows are kept in the handle in INPUT order.  A second call with the other
 *                    biotype adds the remaining families; a call for a biotype no family has does nothing.  The context's
 *                    own batch rows (ka_batch_rows) are replaced, as by any ka_run_encoded_batch.
 *   ka_in_fam_rows_size / ka_in_fam_rows  packed as ka_batch_rows packs them, rows in input order; alnlens_out[n_fam]
 *                    (optional).  While a family is missing: -1 / "ka_in_fam_rows: family 2 has not been run
 *                    (ka_in_fam_run with biotype 1)".
 *   ka_in_fam_stats  out[6]: device ms of the scan [0] and of the encode [1]; kernel launches [2] and host synchronisations
 *                    [3] of create (2 and 2); raw bytes of the batch [4]; wall ms of the ka_in_fam_run calls so far [5].
 */
typedef struct ka_in_fam ka_in_fam;
int  ka_in_tables(int8_t* out3x128);
int  ka_in_detect(const long long* freq128, int* biotype_out);
int  ka_in_order(int n_fam, const int* fam_first, const int* residues, const uint8_t* names, const long long* name_off, int* order_out);
int  ka_in_fam_check(int n_fam, const int* fam_first, const long long* seq_off, long long n_bytes);
int  ka_in_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* text, const long long* seq_off,
                      const uint8_t* names, const long long* name_off, const int* biotype_in, ka_in_fam** out);
void ka_in_fam_destroy(ka_in_fam* h);
int  ka_in_fam_sequences(ka_in_fam* h, int* recs_out);
int  ka_in_fam_families(ka_in_fam* h, int* recs_out, long long* freq_out);
int  ka_in_fam_order(ka_in_fam* h, int* order_out);
long long ka_in_fam_size(ka_in_fam* h);
int  ka_in_fam_encoded(ka_in_fam* h, uint8_t* tree_codes, uint8_t* codes, uint8_t* letters, int* off, int* lens);
int  ka_in_fam_run(ka_in_fam* h, int biotype, const float* subm, const float* scal, int n_anchors, float weight,
                   int realign_iterations, int n_threads, int refine_mode, uint8_t gap_char);
long long ka_in_fam_rows_size(ka_in_fam* h);
int  ka_in_fam_rows(ka_in_fam* h, uint8_t* out, long long cap, int* alnlens_out);
int  ka_in_fam_stats(ka_in_fam* h, double* out);

/*
 * The codon stage (ABI 29): coding DNA of a batch of families, aligned in frame -- translate, align the proteins,
 * backtranslate.  A nucleotide alignment of coding sequences puts one- and two-base gaps where they score well and breaks
 * the reading frame; the reference's positive-selection pipeline works around it, one family at a time on the host:
 *   benchmarks/downstream/positive_selection.py:456-459  "Translate-align-backtranslate to preserve codon reading frame
 *                             Standard DNA alignment can insert 1- or 2-nt gaps that break the codon frame"
 *   :49-66   _translate_dna   "dna_seq = dna_seq.upper()", "if len(dna_seq) % 3 != 0: raise ValueError(...)", "codon =
 *                             dna_seq[i : i + 3]; aa = _CODON_TABLE.get(codon, "X"); if aa != "*": protein.append(aa)"
 *   :69-123  _backtranslate   "original_dna = original_dna.upper()", the same walk keeping the codons whose aa != "*", then
 *                             "if ch == "-": result.append("---") else: ... result.append(codons[codon_idx]); codon_idx += 1"
 *                             and "if codon_idx != len(codons): raise ValueError(...)"
 *   :462-507 the case flow    proteins aligned with seq_type="protein"; "codon_confidence = [c for c in
 *                             aln_result.column_confidence for _ in range(3)]"
 * This stage restates that rule, equal to the reference on letter-only input:
 *   Residues   a sequence's raw bytes pass the input stage's byte rule: letters are residues, punctuation is gap characters
 *              (counted and discarded), other bytes below 128 are dropped, a byte >= 128 is an error.  Residues are
 *              upper-cased.
 *   Codons     residues 3c .. 3c + 2 are codon c.  A residue count that is no multiple of 3 is an error for that sequence.
 *   Code       the standard code over exactly A C G T: index 16a + 4b + c with A 0, C 1, G 2, T 3 into
 *              "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF".  A codon holding any other letter -- N, U
 *              and every ambiguity code included -- translates to X.  U is not T: the reference does not map it, so a codon
 *              with a U is X here too.
 *   Stops      TAA, TAG and TGA are omitted wherever they stand, not only at the end.  A sequence whose every codon is a
 *              stop (or that has no residue) has no protein and is refused, naming family and sequence.
 *   Proteins   the translated proteins are one family each, in the same order, under the caller's names; they go through the
 *              input stage with the biotype forced to protein and from there through ka_in_fam_run, unchanged.
 *   Back       in a protein row of width W a gap byte becomes three gap bytes and the k-th non-gap byte becomes the k-th
 *              non-stop codon of that sequence, upper-cased: a codon row has width 3W.  A row whose non-gap count differs
 *              from the sequence's non-stop codon count is an error, reported before any row is handed out.
 *   A family of one: its protein row is its protein, its codon row its DNA without stop codons.
 *
 * Host only (no context, no GPU):
 *   ka_cod_table     out64: the 64 letters above, '*' for a stop.
 *   ka_cod_fam_check ka_in_fam_check's rules and messages under this stage's name ("ka_cod_fam_check: empty family", ...).
 * The stage:
 *   ka_cod_fam_create  runs the check, uploads the text in one copy and launches twice, back to back: the pack (counts,
 *                    first byte >= 128, the upper-cased residues compacted at seq_off[i] in a plane the size of the text),
 *                    then the translate (the protein plane and the stop-free codon plane, compacted at the same offsets).
 *                    Two launches and one host synchronisation, whatever the batch; then the proteins go to an input stage
 *                    of their own (ka_in_fam_create, biotype 0: its two launches and two synchronisations are its own).
 *                    Fails naming the cause: the check's messages, "ka_cod_fam_create: family 1, sequence 0: byte 0xc3 at
 *                    offset 5", "ka_cod_fam_create: family 1, sequence 2: 301 residues, not a multiple of 3" (the first
 *                    offender in batch order; sequence numbers are within the family), "ka_cod_fam_create: family 0,
 *                    sequence 1 has no protein".  Runs on ctx's device and stream: destroy it before ctx.
 *   ka_cod_fam_sequences  recs_out[numseq * 6] in input order: residues, gap characters, dropped bytes, codons, stop codons,
 *                    X codons.
 *   ka_cod_fam_protein_size / ka_cod_fam_protein  the proteins one after the other in input order (size bytes), and
 *                    off_out[numseq + 1].
 *   ka_cod_fam_run   aligns the proteins (ka_in_fam_run with biotype 0: subm / scal are the protein's) and backtranslates
 *                    the rows.
 *   ka_cod_fam_back  backtranslates rows the caller brings -- a consensus of an ensemble over the same proteins, rows of
 *                    another aligner: protein_rows packed as ka_batch_rows packs them (alnlens[f] + 1 bytes a row, rows in
 *                    input order, n_bytes in all), gap_char their gap byte.  "ka_cod_fam_back: family 0, sequence 1: the row
 *                    holds 6 residues, the sequence 7 codons without stops".  One launch and one synchronisation.
 *                    Both leave protein rows and codon rows in the handle; a later call replaces them, a failed one leaves
 *                    none.
 *   ka_cod_fam_rows_size / ka_cod_fam_rows  the codon rows, packed as ka_batch_rows packs them (3 * alnlen + 1 bytes a
 *                    row, a 0 byte after each), in input order; alnlens_out[n_fam] (optional) the codon widths.  -1 /
 *                    "ka_cod_fam_rows: nothing has been backtranslated" before; a cap too small is refused before anything
 *                    is copied.
 *   ka_cod_fam_protein_rows_size / ka_cod_fam_protein_rows  the protein rows the codon rows were made from, the same way.
 *   ka_cod_fam_stats  out[9]: device ms of the pack [0], the translate [1] and the last backtranslation [2]; kernel launches
 *                    [3] and host synchronisations [4] of create (2 and 1); launches [5] and synchronisations [6] of the
 *                    last backtranslation (1 and 1); raw bytes [7]; wall ms of the ka_cod_fam_run calls so far [8].
 */
typedef struct ka_cod_fam ka_cod_fam;
int  ka_cod_table(uint8_t* out64);
int  ka_cod_fam_check(int n_fam, const int* fam_first, const long long* seq_off, long long n_bytes);
int  ka_cod_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* text, const long long* seq_off,
                       const uint8_t* names, const long long* name_off, ka_cod_fam** out);
void ka_cod_fam_destroy(ka_cod_fam* h);
int  ka_cod_fam_sequences(ka_cod_fam* h, int* recs_out);
long long ka_cod_fam_protein_size(ka_cod_fam* h);
int  ka_cod_fam_protein(ka_cod_fam* h, uint8_t* out, long long* off_out);
int  ka_cod_fam_run(ka_cod_fam* h, const float* subm, const float* scal, int n_anchors, float weight,
                    int realign_iterations, int n_threads, int refine_mode, uint8_t gap_char);
int  ka_cod_fam_back(ka_cod_fam* h, const uint8_t* protein_rows, long long n_bytes, const int* alnlens, uint8_t gap_char);
long long ka_cod_fam_rows_size(ka_cod_fam* h);
int  ka_cod_fam_rows(ka_cod_fam* h, uint8_t* out, long long cap, int* alnlens_out);
long long ka_cod_fam_protein_rows_size(ka_cod_fam* h);
int  ka_cod_fam_protein_rows(ka_cod_fam* h, uint8_t* out, long long cap, int* alnlens_out);
int  ka_cod_fam_stats(ka_cod_fam* h, double* out);

/*
 * The output stage (ABI 30): the finished rows of a batch of families as alignment text -- FASTA, Clustal, MSF, Stockholm
 * with PP lines -- each format written for the whole batch into one buffer by one launch.  What the reference does at its
 * back door, one row and one line at a time:
 *   msa_io.c:668-717          write_msa_fasta: "fprintf(f_ptr,">%s\n", msa->sequences[i]->name);" then the row, "f++; if(f ==
 *                             60){ fprintf(f_ptr, "\n"); f = 0; }" and "if(f){ fprintf(f_ptr,"\n"); }"
 *   python-kalign/io.py:168-173  write_fasta: "handle.write(f">{seq_id}\n")", "for i in range(0, len(seq), line_length):
 *                             handle.write(seq[i : i + line_length] + "\n")" (line_length 80 by default)
 *   msa_io.c:719-866          write_msa_clu: "snprintf(ol->line, line_length,"Kalign (%s) multiple sequence alignment",
 *                             KALIGN_PACKAGE_VERSION);", an empty line, then per row and block "for(j = c;j <
 *                             max_name_len+5;j++){ ol->line[j] = ' '; }" and up to 60 bytes of the row; with row 0 of each
 *                             block a line "ol->line[0] = '\n'; ol->line[1] = 0;" of seq_id numseq; all lines sorted by
 *                             block, then seq_id (sort_out_lines, :1293) and printed with "fprintf(f_ptr, "%s\n", ol->line);"
 *   msa_io.c:869-1150         write_msa_msf: "aln_len = msa->sequences[0]->len;", the banner, "" and
 *                             " %s  MSF: %d  Type: %c  %s  Check: %d  .." (basename or "stdout", aln_len, "msa->L ==
 *                             ALPHA_defPROTEIN ? 'P' : 'N'", the date "%B %d, %Y %H:%M", GCGMultchecksum), "", per row
 *                             " Name: %-*.*s  Len:  %5d  Check: %4d  Weight: %.2f" (max_name_len twice, the name, aln_len,
 *                             "GCGchecksum(msa->sequences[i]->seq, msa->sequences[i]->len)", 1.0), "", "//", "", then
 *                             "aln_len = msa->alnlen;" and write_msa_clu's blocks
 *   msa_misc.c:12-33          GCGMultchecksum: "chk = (chk + GCGchecksum(...)) % 10000;"; GCGchecksum: "chk = (chk + (i % 57 +
 *                             1) * (toupper((int) seq[i]))) % 10000;"
 *   python-kalign/io.py:239-243  _conf_to_pp_char: "if conf >= 0.95: return "*"" else "return str(int(conf * 10))"
 *   python-kalign/io.py:292-317  write_stockholm with confidences: "# STOCKHOLM 1.0\n", per row "f"{seq_id:<{max_id}}
 *                             {seq}\n"" (three spaces) and, with residue confidences, "if ch == "-" or ch == ".":
 *                             pp.append(".")" else the PP character, "f"#=GR {seq_id:<{max_id}} PP {pp_str}\n""; with column
 *                             confidences "f"#=GC {'PP_cons':<{pp_label_len}}   {pp_cons}\n"" with pp_label_len = max(max_id,
 *                             7); "//\n"
 * This stage writes the same bytes:
 *   Rows       packed as ka_sum_fam_create takes them (a row of W columns W + 1 bytes), in the caller's order, under
 *              ka_sum_fam_check's rules.  A byte of a row equal to gap_char is a gap, every other byte a character, taken as an
 *              unsigned byte.  Only MSF's character counts ask.
 *   Names      packed as the input stage takes them (names, name_off[numseq + 1]), or both NULL: family f's rows are named
 *              seq0, seq1, ..., python-kalign's default.  A name is 1 to 255 bytes of printable ASCII (32..126); the
 *              reference keeps MSA_NAME_LEN = 256 with the terminator.
 *   Texts      every format is written for the whole batch into `out` (cap bytes), family after family; fam_off_out[n_fam +
 *              1] (may be NULL) says where each family's text lies, fam_off_out[n_fam] is the size.  The _size call gives the
 *              size alone, or -1.
 *   FASTA      line_length >= 1: per row ">name\n" and the row in pieces of line_length bytes, each followed by "\n".  60 is
 *              write_msa_fasta, 80 kalign.io.write_fasta's default.
 *   Clustal    `header` (at most 255 bytes; the reference's is "Kalign (<version>) multiple sequence alignment"), an empty line,
 *              then max(1, ceil(W / 60)) blocks: per row the name padded with spaces to the family's longest name + 5 and up
 *              to 60 bytes of the row, then two newline bytes (the reference's stored "\n" printed with "%s\n").  A width that
 *              is a multiple of 60 opens no empty block.
 *   MSF        the reference's arithmetic as it stands: finalise_alignment never sets seq->len to the alignment length, so
 *              with chars_i the characters of row i, "MSF:" and every "Len:" carry chars_0, a row's "Check:" is GCGchecksum
 *              over the first chars_i BYTES of the aligned row i, gaps included, and the file's "Check:" is their sum modulo
 *              10000.  The blocks are Clustal's (no space every ten letters, whatever the reference's comment says).  Per family
 *              a title (1 to 255 printable bytes; titles / title_off[n_fam + 1] packed like names: the file's basename, or
 *              "stdout") and a biotype, 0 protein or 1 DNA; per call the date string (1 to 63 printable bytes).  The library
 *              never reads the clock.  Banner and type letter are what the reference's CLI writes after a run, and it writes
 *              "!!NA_MULTIPLE_ALIGNMENT 1.0" and "Type: N" for a protein and for a DNA family alike: after a run msa->L is
 *              neither ALPHA_defPROTEIN nor ALPHA_redPROTEIN (recorded in tests/golden/out_prot.npz and out_dna.npz).
 *   Stockholm  residue_conf: float32, N_f * W_f per family, packed like the rows without the pad byte; column_conf: float32,
 *              W_f per family; either may be NULL, not both: without confidences the reference writes through Biopython, which
 *              this stage does not restate.  Lines are not wrapped, and the "#=GR" lines do not line up with the rows, as in
 *              the reference.  A PP byte is '.' where the row's byte is '-' or '.' -- the reference's test, NOT the handle's
 *              gap_char -- and the confidence there is not looked at.  Elsewhere, with v the float's value as a double: '*'
 *              when v >= 0.95, else the digit (int)(v * 10.0).  PP_cons uses the same rule without the gap test.  A NaN or a
 *              value outside [0, 1] (-0.0 is inside) would make the reference print two characters or raise; here the call
 *              fails naming the first offender in batch order -- families in order, in a family its residue confidences row
 *              after row, then its column confidences -- and `out` is zeroed over the text's size: no text is handed out.
 *
 * Host only (no context, no GPU):
 *   ka_out_pp_char   the PP byte of a confidence, or -1 for a NaN and a value outside [0, 1].
 *   ka_out_fam_check ka_sum_fam_check's rules and messages under this stage's name ("ka_out_fam_check: empty family", ...),
 *                    then the names: "ka_out_fam_check: name_off does not ascend", "ka_out_fam_check: family 1, sequence 2:
 *                    empty name", "ka_out_fam_check: family 1, sequence 2: name of 256 bytes; a name holds 1 to 255",
 *                    "ka_out_fam_check: family 1, sequence 2: name byte 0x1f at offset 3; a name is printable ASCII (32..126)".
 *   ka_out_fam_text_sizes  the closed forms alone: fam_off_out[n_fam + 1] of FASTA (format 0, param line_length), Clustal (1,
 *                    param the header's bytes) or Stockholm (2, param 1 residue, 2 column, 3 both confidences) for families of
 *                    these sizes, widths and name lengths (name_off NULL: the default names).  An MSF text's size depends on
 *                    its records and has no closed form.
 * The stage:
 *   ka_out_fam_create  runs the check and uploads rows and names once; every format is written from them.  Nothing is
 *                    launched.  Runs on ctx's device and stream: destroy it before ctx.
 *   ka_out_fam_fasta / ka_out_fam_clustal / ka_out_fam_stockholm  the size is a closed form on the host; a cap below it is
 *                    refused before anything is launched ("ka_out_fam_fasta: 99 bytes do not hold the text (100)").  Then the
 *                    call's tables go up (a record and an offset per family, FASTA: an offset per row, the header), one launch
 *                    fills the text -- a lane per aligned dword, assembled from as many lines as it spans -- and the text comes
 *                    down: 1 launch and 1 host synchronisation per call, whatever the number of families.  Refusals:
 *                    "ka_out_fam_fasta: line_length 0; a line holds one column at least", "ka_out_fam_clustal: header of 300
 *                    bytes; it holds 255 at most", "ka_out_fam_stockholm: without confidences the reference writes Stockholm
 *                    through Biopython, which this stage does not restate: give residue_conf, column_conf or both",
 *                    "ka_out_fam_stockholm: family 1, sequence 2, column 5: confidence 1.00010002 outside [0, 1]",
 *                    "ka_out_fam_stockholm: family 1, column 5: column confidence nan outside [0, 1]".  A refused call leaves
 *                    the handle usable.
 *   ka_out_fam_msf_records  recs_out[numseq * 2]: characters and prefix checksum of every row; fam_check_out[n_fam]: the
 *                    families' checks (each optional).  They come from a row pass on the device, a wave per row: 1 launch and
 *                    1 synchronisation, once per handle; the records stay on the host.
 *   ka_out_fam_msf_size / ka_out_fam_msf  run the row pass when the handle has not, format the headers on the host from its
 *                    records with the reference's format strings, and upload them; then as above.  The first MSF call on a
 *                    handle counts 2 launches and 2 synchronisations (the row pass, wherever it ran, counts with the first
 *                    writer after it), later ones 1 and 1.  The size depends on the records, so the cap is checked after the
 *                    row pass and before the fill.  Refusals: "ka_out_fam_msf: family 0: title of 0 bytes; it holds 1 to 255",
 *                    "ka_out_fam_msf: family 0: title holds a byte that is not printable ASCII (32..126)", "ka_out_fam_msf:
 *                    family 0: biotype 2 is not 0 (protein) or 1 (DNA)", "ka_out_fam_msf: the date of 0 bytes; it holds 1 to
 *                    63", "ka_out_fam_msf: the date holds a byte that is not printable ASCII (32..126)".
 *   ka_out_fam_stats out4: device ms of the row pass [0] and of the last fill [1]; kernel launches [2] and host
 *                    synchronisations [3] of the last writer.
 */
typedef struct ka_out_fam ka_out_fam;
int  ka_out_pp_char(float confidence);
int  ka_out_fam_check(int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens, const uint8_t* names, const long long* name_off);
int  ka_out_fam_text_sizes(int n_fam, const int* fam_first, const int* alnlens, const long long* name_off, int format, int param,
                           long long* fam_off_out);
int  ka_out_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens, int gap_char,
                       const uint8_t* names, const long long* name_off, ka_out_fam** out);
void ka_out_fam_destroy(ka_out_fam* h);
long long ka_out_fam_fasta_size(ka_out_fam* h, int line_length);
int  ka_out_fam_fasta(ka_out_fam* h, int line_length, uint8_t* out, long long cap, long long* fam_off_out);
long long ka_out_fam_clustal_size(ka_out_fam* h, const char* header);
int  ka_out_fam_clustal(ka_out_fam* h, const char* header, uint8_t* out, long long cap, long long* fam_off_out);
int  ka_out_fam_msf_records(ka_out_fam* h, int* recs_out, int* fam_check_out);
long long ka_out_fam_msf_size(ka_out_fam* h, const uint8_t* titles, const long long* title_off, const int* biotypes, const char* date);
int  ka_out_fam_msf(ka_out_fam* h, const uint8_t* titles, const long long* title_off, const int* biotypes, const char* date, uint8_t* out,
                    long long cap, long long* fam_off_out);
long long ka_out_fam_stockholm_size(ka_out_fam* h, int has_residue_conf, int has_column_conf);
int  ka_out_fam_stockholm(ka_out_fam* h, const float* residue_conf, const float* column_conf, uint8_t* out, long long cap,
                          long long* fam_off_out);
int  ka_out_fam_stats(ka_out_fam* h, double* out4);

#ifdef __cplusplus
}
#endif
#endif
