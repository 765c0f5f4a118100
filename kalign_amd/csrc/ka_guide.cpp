// Guide tree: build_tree_kmeans (reference lib/src/bisectingKmeans.c:177-271) -- the stage that produces the task
// list and msa->seq_distances the dispatcher consumes.
//
// The distances (N x 32 against the anchors, then all pairs inside every leaf cluster) are the two GPU batches
// (ka_bpm_batch); what sits between them -- anchor choice, bisecting k-means on the N x 32 matrix, UPGMA inside
// clusters of < 50 sequences, node labels, task list -- is small, branchy host work and stays on the host, in the
// reference's fp32 evaluation order so that the tree is the same tree, bit for bit.
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "kalign_amd.h"
#include "ka_ctx.h"          // ka_ctx_device_stream, the family table's rule (its fail() sets what ka_fail_message sets)
#include "ka_kmeans.h"

namespace {

constexpr int KA_UPGMA_BELOW = 50;            // KALIGN_KMEANS_UPGMA_THRESHOLD, reference CMakeLists.txt:71
constexpr int KA_MAX_ANCHORS = 32;            // pick_anchor.c:25

struct Node { int left = -1, right = -1, id = -1; };

struct Tree {
        std::vector<Node> nodes;
        int add(int l, int r, int id) { nodes.push_back(Node{ l, r, id }); return (int)nodes.size() - 1; }
};

// pick_anchor.c:34-70: sort by length, longest first, and take every (numseq / n)-th.  The reference's comparator
// never reports equality, so the order of equal lengths is whatever the C library's qsort makes of it: use the same
// qsort on the same element type (pointers to {len, id}) so that both see the same comparisons.
struct LenId { int len, id; };
int by_len_desc(const void* a, const void* b)
{
        const LenId* const* x = (const LenId* const*)a;
        const LenId* const* y = (const LenId* const*)b;
        return ((*x)->len > (*y)->len) ? -1 : 1;
}

void pick_anchors(int numseq, const int* lens, std::vector<int>& anchors)
{
        const int n = std::min(KA_MAX_ANCHORS, numseq);
        std::vector<LenId> recs(numseq);
        std::vector<LenId*> ptr(numseq);
        for (int i = 0; i < numseq; i++) { recs[i] = LenId{ lens[i], i }; ptr[i] = &recs[i]; }
        qsort(ptr.data(), numseq, sizeof(LenId*), by_len_desc);
        const int stride = numseq / n;
        anchors.resize(n);
        for (int i = 0; i < n; i++) anchors[i] = ptr[(size_t)i * stride]->id;
}

// d_estimation's length term (sequence_distance.c:66-69,118-120); the quotient is formed in double there
inline float with_length_term(int dist, int l1, int l2)
{
        const int s = (l1 + l2) / 2;
        const float add = (float)((10000.0 < (double)s ? 10000.0 : (double)s) / 10000.0);
        float d = (float)dist;
        d += add;
        return d;
}

// edist_256 (euclidean_dist.c): eight running lane sums, then (l0+l4 + l1+l5) + (l2+l6 + l3+l7), then sqrtf.
// `a`, `b` hold `padded` floats, zero beyond the anchors.
inline float edist(const float* a, const float* b, int padded)
{
        float lane[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        for (int i = 0; i < padded; i += 8)
                for (int k = 0; k < 8; k++) {
                        float t = a[i + k] - b[i + k];
                        t = t * t;
                        lane[k] = lane[k] + t;
                }
        const float v0 = lane[0] + lane[4], v1 = lane[1] + lane[5], v2 = lane[2] + lane[6], v3 = lane[3] + lane[7];
        const float s01 = v0 + v1, s23 = v2 + v3;
        return sqrtf(s01 + s23);
}

inline int cmp_floats(float a, float b)          // bisectingKmeans.c:63-73
{
        const float epsilon = 1e-6f;
        if (fabsf(a - b) < epsilon) return 0;
        return a > b ? 1 : -1;
}

struct Split { std::vector<int> sl, sr; float score = FLT_MAX; };

// What a split2 went through, for the tests (ka_debug_kmeans_host): the set's centroid, min(dl, dr) of every sample in the
// last iteration, and the counters that show which branches an input reached.
struct SplitTrace {
        std::vector<float> w, mind;
        int iterations = 0, parity_total = 0, parity_last = 0;      // samples decided by the index parity rule (c == 0)
        bool degenerate = false;
};

// split2 (bisectingKmeans.c:766-971): 2-means from one seed sample and its mirror image through the centroid.
// TRACE: the tests' instantiation fills `tr`; the product's (TRACE = false) carries none of it.
template <bool TRACE = false>
void split2(const float* dm, int padded, const std::vector<int>& samples, int num_anchors, int seed_pick, Split& res, SplitTrace* tr = nullptr)
{
        const int num_samples = (int)samples.size();
        std::vector<float> w(padded, 0.0f), wl(padded, 0.0f), wr(padded, 0.0f), cl(padded, 0.0f), cr(padded, 0.0f);
        for (int i = 0; i < num_samples; i++) {
                const float* row = dm + (size_t)samples[i] * padded;
                for (int j = 0; j < num_anchors; j++) w[j] += row[j];
        }
        for (int j = 0; j < num_anchors; j++) w[j] /= (float)num_samples;
        if (TRACE) { tr->w = w; tr->mind.assign(num_samples, 0.0f); }
        {
                const float* row = dm + (size_t)samples[seed_pick] * padded;
                for (int j = 0; j < num_anchors; j++) cl[j] = row[j];
                for (int j = 0; j < num_anchors; j++) cr[j] = w[j] - (cl[j] - w[j]);
        }
        res.sl.resize(num_samples);
        res.sr.resize(num_samples);
        int num_l = 0, num_r = 0;
        float score = 0.0f;
        float *pcl = cl.data(), *pcr = cr.data(), *pwl = wl.data(), *pwr = wr.data();
        for (int stop = 0; stop < 500; stop++) {
                num_l = num_r = 0;
                for (int i = 0; i < num_anchors; i++) { pwr[i] = 0.0f; pwl[i] = 0.0f; }
                score = 0.0f;
                if (TRACE) { tr->iterations++; tr->parity_last = 0; }
                for (int i = 0; i < num_samples; i++) {
                        const int s = samples[i];
                        const float* row = dm + (size_t)s * padded;
                        const float dl = edist(row, pcl, padded);
                        const float dr = edist(row, pcr, padded);
                        score += (dl < dr) ? dl : dr;
                        const int c = cmp_floats(dr, dl);
                        if (TRACE) { tr->mind[i] = (dl < dr) ? dl : dr; if (c == 0) { tr->parity_total++; tr->parity_last++; } }
                        float* acc;
                        if (c == -1 || (c == 0 && (i & 1))) { acc = pwr; res.sr[num_r++] = s; }
                        else { acc = pwl; res.sl[num_l++] = s; }
                        for (int j = 0; j < num_anchors; j++) acc[j] += row[j];
                }
                if (num_l == 0 || num_r == 0) {                  // degenerate: cut the list in the middle, score 0
                        if (TRACE) tr->degenerate = true;
                        score = 0.0f;
                        num_l = num_r = 0;
                        for (int i = 0; i < num_samples / 2; i++) res.sl[num_l++] = samples[i];
                        for (int i = num_samples / 2; i < num_samples; i++) res.sr[num_r++] = samples[i];
                        break;
                }
                for (int j = 0; j < num_anchors; j++) { pwl[j] /= (float)num_l; pwr[j] /= (float)num_r; }
                bool moved = false;
                for (int j = 0; j < num_anchors; j++)
                        if (cmp_floats(pwl[j], pcl[j]) != 0 || cmp_floats(pwr[j], pcr[j]) != 0) { moved = true; break; }
                if (!moved) break;
                std::swap(pcl, pwl);
                std::swap(pcr, pwr);
        }
        res.sl.resize(num_l);
        res.sr.resize(num_r);
        res.score = score;
}

struct Builder {
        int numseq = 0, num_anchors = 0, padded = 0;
        const float* dm = nullptr;
        int n_threads = 1;
};

// A subtree under construction.  Children are either finished subtrees or leaf clusters waiting for their
// pairwise distances.
struct Sub {
        std::unique_ptr<Sub> l, r;
        std::vector<int> cluster;            // non-empty: a leaf cluster (l, r empty)
};

// bisecting_kmeans (bisectingKmeans.c:273-402)
std::unique_ptr<Sub> bisect(const Builder& B, std::vector<int> samples, int depth)
{
        std::unique_ptr<Sub> out(new Sub());
        const int num_samples = (int)samples.size();
        if (num_samples < KA_UPGMA_BELOW) { out->cluster = std::move(samples); return out; }
        const int tries = std::min(40, num_samples);
        const int step = num_samples / tries;
        Split best;
        bool have_best = false;
        for (int i = 0; i < tries; i += 4) {
                Split cand[4];
                if (B.n_threads > 1 && num_samples >= 128) {     // the reference: four OpenMP tasks (:325-340)
                        std::future<void> f[3];
                        bool started[3] = { false, false, false };
                        for (int k = 1; k < 4; k++) {
                                try {
                                        f[k - 1] = std::async(std::launch::async, [&, k] { split2(B.dm, B.padded, samples, B.num_anchors, (i + k) * step, cand[k]); });
                                        started[k - 1] = true;
                                } catch (const std::system_error&) {}     // no thread to be had: this candidate runs here
                        }
                        split2(B.dm, B.padded, samples, B.num_anchors, i * step, cand[0]);
                        for (int k = 0; k < 3; k++) {
                                if (started[k]) f[k].get();
                                else split2(B.dm, B.padded, samples, B.num_anchors, (i + k + 1) * step, cand[k + 1]);
                        }
                } else {
                        for (int k = 0; k < 4; k++) split2(B.dm, B.padded, samples, B.num_anchors, (i + k) * step, cand[k]);
                }
                int change = 0;
                for (int k = 0; k < 4; k++)
                        if (!have_best || best.score > cand[k].score) { best = std::move(cand[k]); have_best = true; change++; }
                if (!change) break;
        }
        samples.clear();
        samples.shrink_to_fit();
        std::future<std::unique_ptr<Sub>> fut;
        bool forked = false;
        // (a degenerate input can peel one sequence off per split: bound the recursion -- the C ABI wrapper turns
        // this into KA_FAIL -- instead of overflowing the stack)
        if (depth > 4096) throw std::runtime_error("bisecting k-means degenerated (recursion deeper than 4096)");
        if (depth < 30 && (1 << depth) < B.n_threads) {                // the two halves are independent (the reference: OpenMP tasks)
                try {
                        fut = std::async(std::launch::async, [&] { return bisect(B, std::move(best.sl), depth + 1); });
                        forked = true;
                } catch (const std::system_error&) {}             // no thread to be had: serial
        }
        if (forked) {
                out->r = bisect(B, std::move(best.sr), depth + 1);
                out->l = fut.get();
        } else {
                out->l = bisect(B, std::move(best.sl), depth + 1);
                out->r = bisect(B, std::move(best.sr), depth + 1);
        }
        return out;
}

// upgma (bisectingKmeans.c:974-1053) on an n x n matrix whose upper triangle is valid; returns the root node index
int upgma(Tree& T, std::vector<float>& dm, const std::vector<int>& samples)
{
        const int n = (int)samples.size();
        std::vector<int> active(n, 1), tree(n);
        for (int i = 0; i < n; i++) tree[i] = T.add(-1, -1, samples[i]);
        int node_a = 0, node_b = 0;
        for (int merges = 0; merges < n - 1; merges++) {
                float best = FLT_MAX;
                for (int i = 0; i < n - 1; i++) {
                        if (!active[i]) continue;
                        for (int j = i + 1; j < n; j++)
                                if (active[j] && dm[(size_t)i * n + j] < best) { best = dm[(size_t)i * n + j]; node_a = i; node_b = j; }
                }
                tree[node_a] = T.add(tree[node_a], tree[node_b], -1);
                tree[node_b] = -1;
                active[node_b] = 0;
                for (int j = n; j--;)
                        if (j != node_b) dm[(size_t)node_a * n + j] = (dm[(size_t)node_a * n + j] + dm[(size_t)node_b * n + j]) * 0.5f + 0.001f;
                dm[(size_t)node_a * n + node_a] = 0.0f;
                for (int j = n; j--;) dm[(size_t)j * n + node_a] = dm[(size_t)node_a * n + j];
        }
        return tree[node_a];
}

// label_internal + create_tasks + sort_tasks(TASK_ORDER_TREE) (bisectingKmeans.c:1067-1115, task.c:114-136):
// internal nodes numbered in post-order from numseq, one task per internal node, c ascending.  Returns the task count.
int emit_tasks(Tree& T, int top, int numseq, int* tasks_abc)
{
        int label = numseq, n_tasks = 0;
        struct Walk { int node; int state; };
        std::vector<Walk> ws;
        ws.push_back(Walk{ top, 0 });
        while (!ws.empty()) {
                Walk& w = ws.back();
                Node& nd = T.nodes[w.node];
                if (nd.left < 0) { ws.pop_back(); continue; }
                if (w.state == 0) { w.state = 1; ws.push_back(Walk{ nd.left, 0 }); continue; }
                if (w.state == 1) { w.state = 2; ws.push_back(Walk{ nd.right, 0 }); continue; }
                nd.id = label++;
                tasks_abc[3 * n_tasks] = T.nodes[nd.left].id;
                tasks_abc[3 * n_tasks + 1] = T.nodes[nd.right].id;
                tasks_abc[3 * n_tasks + 2] = nd.id;
                n_tasks++;
                ws.pop_back();
        }
        return n_tasks;
}

void collect_leaves(Sub* root, std::vector<Sub*>& out)
{
        std::vector<Sub*> st(1, root);                   // iterative pre-order, left before right
        while (!st.empty()) {
                Sub* s = st.back(); st.pop_back();
                if (!s->l) { out.push_back(s); continue; }
                st.push_back(s->r.get());
                st.push_back(s->l.get());
        }
}

}  // namespace

int ka_fail_message(const char* m);      // ka_api.cpp: sets what ka_last_error() returns

// the library's own distance source (ka_bpm_batch) has already said why: keep its text
static int dist_failed(const char* who)
{
        const std::string inner = ka_last_error();
        return ka_fail_message((std::string(who) + ": the distance source failed" + (inner.empty() ? std::string() : ": " + inner)).c_str());
}

static int guide_forest_from(const char* who, int n_fam, const int* fam_first, const int* lens, ka_dist_fn dist, void* user, int n_threads,
                             const float* dm_scale, int* tasks_abc, int* n_tasks_out, float* seq_distances);


// The 2-means bisection on the device (ka_kmeans.hip) for the callers that have one: ka_guide_tree sets the device and stream
// of its context here for the duration of the call.  KA_KMEANS in the environment: "0" host, "1" device whatever the size;
// default: the device from 2048 sequences (below that the host's 40 x 2-means take less than the launches).
namespace {
struct KmDevice { bool on = false; int device = 0; hipStream_t stream = nullptr; };
thread_local KmDevice g_km;
double g_last_bisect_ms = 0.0;
int g_last_bisect_device = 0;
}
extern "C" double ka_guide_last_bisect_ms(int* on_device)
{
        if (on_device) *on_device = g_last_bisect_device;
        return g_last_bisect_ms;
}

extern "C" int ka_guide_tree_from(int numseq, const int* lens, ka_dist_fn dist, void* user, int n_threads,
                                  const float* dm_scale, int* tasks_abc, float* seq_distances)
{
        try {                                            // no exception may cross the C ABI
                if (numseq < 2 || !lens || !dist || !tasks_abc) return ka_fail_message("ka_guide_tree_from: bad arguments");
                const int fam_first[2] = { 0, numseq };
                return guide_forest_from("ka_guide_tree_from", 1, fam_first, lens, dist, user, n_threads, dm_scale, tasks_abc, nullptr, seq_distances);
        } catch (const std::bad_alloc&) {
                return ka_fail_message("ka_guide_tree_from: out of memory");
        } catch (const std::exception& e) {
                return ka_fail_message((std::string("ka_guide_tree_from: ") + e.what()).c_str());
        }
}

// The guide trees of a batch of families: sequences fam_first[f] .. fam_first[f + 1] - 1 are family f.  The three phases of
// build_tree_kmeans run over ALL families before the next one starts, so that the distance source is called at most twice
// however many families there are; what a family does between the calls is what it does alone, on its own data.
extern "C" int ka_guide_forest_from(int n_fam, const int* fam_first, const int* lens, ka_dist_fn dist, void* user, int n_threads,
                                    const float* dm_scale, int* tasks_abc, int* n_tasks_out, float* seq_distances)
{
        try {
                if (n_fam < 1 || !fam_first || !lens || !dist || !tasks_abc) return ka_fail_message("ka_guide_forest_from: bad arguments");
                return guide_forest_from("ka_guide_forest_from", n_fam, fam_first, lens, dist, user, n_threads, dm_scale, tasks_abc, n_tasks_out, seq_distances);
        } catch (const std::bad_alloc&) {
                return ka_fail_message("ka_guide_forest_from: out of memory");
        } catch (const std::exception& e) {
                return ka_fail_message((std::string("ka_guide_forest_from: ") + e.what()).c_str());
        }
}

namespace {
// One family between the phases.  Indices are the family's own (0 .. n - 1) except in the pair lists handed to the distance source.
struct Fam {
        int first = 0, n = 0, A = 0, padded = 0;
        bool km_dev = false;                         // its bisection runs on the device (on the calling thread)
        std::vector<int> anchors;
        std::vector<float> dm;
        std::unique_ptr<Sub> root;
        std::vector<Sub*> leaves;
        std::vector<size_t> first_pair;              // of every leaf cluster, from p2
        size_t p1 = 0, p2 = 0;                       // the family's first pair in the anchor batch / the cluster batch
        std::vector<int> tasks;                      // 3 * (n - 1), nodes numbered as for the family alone
};

// fn(f) for every f < n on up to n_threads threads; the first exception is thrown again here
template <typename F>
void for_each_family(int n, int n_threads, F fn)
{
        if (n_threads < 2 || n < 2) { for (int f = 0; f < n; f++) fn(f); return; }
        std::atomic<int> next(0);
        std::exception_ptr err;
        std::mutex err_lock;
        auto work = [&] {
                for (int f; (f = next.fetch_add(1)) < n;) {
                        try { fn(f); }
                        catch (...) { std::lock_guard<std::mutex> g(err_lock); if (!err) err = std::current_exception(); }
                }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < std::min(n_threads, n); t++) {
                try { pool.emplace_back(work); } catch (const std::system_error&) { break; }      // no thread to be had: fewer
        }
        work();
        for (auto& t : pool) t.join();
        if (err) std::rethrow_exception(err);
}
}  // namespace

static int guide_forest_from(const char* who, int n_fam, const int* fam_first, const int* lens, ka_dist_fn dist, void* user, int n_threads,
                             const float* dm_scale, int* tasks_abc, int* n_tasks_out, float* seq_distances)
{
        const std::string me(who);
        if (ka_fam_check_first(me, n_fam, fam_first)) return KA_FAIL;
        const int numseq = fam_first[n_fam];
        for (int i = 0; i < numseq; i++)
                if (lens[i] < 1) return ka_fail_message((me + ": zero-length sequence").c_str());
        n_threads = std::max(1, n_threads);

        // ---- anchors and the N x A distance matrix of every family (pick_anchor, d_estimation with pair = 0): ONE batch ----
        std::vector<Fam> fams(n_fam);
        size_t total = 0;
        int n_trees = 0;
        for (int f = 0; f < n_fam; f++) {
                Fam& F = fams[f];
                F.first = fam_first[f]; F.n = fam_first[f + 1] - fam_first[f];
                if (F.n < 2) continue;                           // one sequence: no tree
                n_trees++;
                pick_anchors(F.n, lens + F.first, F.anchors);
                F.A = (int)F.anchors.size();
                F.padded = ((F.A + 7) / 8) * 8;
                F.p1 = total;
                total += (size_t)F.n * F.A;
        }
        if (total > (size_t)INT32_MAX) return ka_fail_message((me + ": more than 2^31 anchor distances in one batch").c_str());
        std::vector<int> ia(total), ib(total), d(total);
        for (const Fam& F : fams)
                for (int i = 0; i < F.n && F.A; i++)
                        for (int j = 0; j < F.A; j++) { ia[F.p1 + (size_t)i * F.A + j] = F.first + i; ib[F.p1 + (size_t)i * F.A + j] = F.first + F.anchors[j]; }
        if (total && dist(user, (int)total, ia.data(), ib.data(), d.data())) return dist_failed(who);

        // ---- per family: the matrix, then bisecting k-means down to clusters of < 50 sequences ----
        // (the threads go to the families when there are several, into the one family's bisection when there is one)
        const int inner_threads = n_trees > 1 ? 1 : n_threads;
        const char* km_env = getenv("KA_KMEANS");
        std::vector<size_t> scale_off(n_fam + 1, 0);             // dm_scale: the families' blocks, n x min(32, n) each
        for (int f = 0; f < n_fam; f++) scale_off[f + 1] = scale_off[f] + (size_t)fams[f].n * std::min(KA_MAX_ANCHORS, fams[f].n);
        auto matrix = [&](Fam& F, int f) {
                const int* flen = lens + F.first;
                F.dm.assign((size_t)F.n * F.padded, 0.0f);
                for (int i = 0; i < F.n; i++)
                        for (int j = 0; j < F.A; j++) F.dm[(size_t)i * F.padded + j] = with_length_term(d[F.p1 + (size_t)i * F.A + j], flen[i], flen[F.anchors[j]]);
                // build_tree_kmeans_noisy (:103-115): the caller's multiplicative noise on the anchor distances
                if (dm_scale)
                        for (int i = 0; i < F.n; i++)
                                for (int j = 0; j < F.A; j++) F.dm[(size_t)i * F.padded + j] *= dm_scale[scale_off[f] + (size_t)i * F.A + j];
        };
        auto clusters = [&](Fam& F) {
                collect_leaves(F.root.get(), F.leaves);
                F.first_pair.assign(F.leaves.size() + 1, 0);
                for (size_t k = 0; k < F.leaves.size(); k++) {
                        const size_t n = F.leaves[k]->cluster.size();
                        F.first_pair[k + 1] = F.first_pair[k] + n * (n - 1) / 2;
                }
        };
        const auto t_bisect = std::chrono::steady_clock::now();
        g_last_bisect_device = 0;
        for (int f = 0; f < n_fam; f++) {                        // the device's bisections first, from this thread
                Fam& F = fams[f];
                F.km_dev = F.n >= 2 && g_km.on && F.A == 32 && F.padded == 32 && (km_env ? atoi(km_env) != 0 : F.n >= 2048);
                if (!F.km_dev) continue;
                g_last_bisect_device = 1;
                matrix(F, f);
                std::vector<KaKmNode> kn;
                std::string why;
                if (ka_kmeans_device(g_km.device, g_km.stream, F.dm.data(), F.n, kn, why)) return ka_fail_message(("ka_guide_tree: " + why).c_str());
                // the device's node table as the builder's tree (iteratively: lopsided splits make it deep)
                std::vector<std::unique_ptr<Sub>> made(kn.size());
                for (size_t k = kn.size(); k--;) {                  // children have larger indices than their parent
                        made[k].reset(new Sub());
                        if (kn[k].left < 0) made[k]->cluster = std::move(kn[k].cluster);
                        else { made[k]->l = std::move(made[kn[k].left]); made[k]->r = std::move(made[kn[k].right]); }
                }
                F.root = std::move(made[0]);
                clusters(F);
        }
        for_each_family(n_fam, n_trees > 1 ? n_threads : 1, [&](int f) {
                Fam& F = fams[f];
                if (F.n < 2 || F.km_dev) return;
                matrix(F, f);
                Builder B;
                B.numseq = F.n; B.num_anchors = F.A; B.padded = F.padded; B.dm = F.dm.data(); B.n_threads = inner_threads;
                std::vector<int> all(F.n);
                for (int i = 0; i < F.n; i++) all[i] = i;
                F.root = bisect(B, std::move(all), 0);
                clusters(F);
        });
        g_last_bisect_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_bisect).count();

        // ---- all pairs inside every leaf cluster of every family in ONE batch (d_estimation with pair = 1): the value the
        //      reference keeps for i < j is the one it computes last, calc_distance(seq[samples[j]], seq[samples[i]]) ----
        total = 0;
        for (Fam& F : fams) { F.p2 = total; if (F.n >= 2) total += F.first_pair.back(); }
        if (total > (size_t)INT32_MAX) return ka_fail_message((me + ": more than 2^31 in-cluster distances in one batch").c_str());
        ia.assign(total, 0); ib.assign(total, 0); d.assign(total, 0);
        for (const Fam& F : fams)
                for (size_t k = 0; k < F.leaves.size(); k++) {
                        const std::vector<int>& s = F.leaves[k]->cluster;
                        size_t p = F.p2 + F.first_pair[k];
                        for (size_t i = 0; i < s.size(); i++)
                                for (size_t j = i + 1; j < s.size(); j++, p++) { ia[p] = F.first + s[j]; ib[p] = F.first + s[i]; }
                }
        if (total && dist(user, (int)total, ia.data(), ib.data(), d.data())) return dist_failed(who);

        // ---- per family: UPGMA inside the clusters, then labels and tasks in post-order (label_internal, create_tasks,
        //      sort_tasks(TASK_ORDER_TREE): c ascending == post-order), and msa->seq_distances ----
        std::atomic<int> bad_count(0);
        for_each_family(n_fam, n_threads, [&](int f) {
                Fam& F = fams[f];
                if (F.n < 2) { if (seq_distances) seq_distances[F.first] = 0.0f; return; }
                const int* flen = lens + F.first;
                Tree T;
                std::vector<int> leaf_root(F.leaves.size());
                for (size_t k = 0; k < F.leaves.size(); k++) {
                        const std::vector<int>& s = F.leaves[k]->cluster;
                        const int n = (int)s.size();
                        std::vector<float> pd((size_t)n * n, 0.0f);
                        size_t p = F.p2 + F.first_pair[k];
                        for (int i = 0; i < n; i++)
                                for (int j = i + 1; j < n; j++, p++) {
                                        const float v = with_length_term(d[p], flen[s[j]], flen[s[i]]);
                                        pd[(size_t)i * n + j] = v;
                                        pd[(size_t)j * n + i] = v;
                                }
                        leaf_root[k] = upgma(T, pd, s);
                }
                // stitch the k-means levels above the clusters (iteratively: the recursion can be N deep when splits are lopsided)
                size_t next_leaf = 0;
                struct Frame { Sub* s; int state; int l; };
                std::vector<Frame> st;
                std::vector<int> done;           // node indices of finished subtrees
                st.push_back(Frame{ F.root.get(), 0, -1 });
                while (!st.empty()) {
                        Frame& fr = st.back();
                        if (!fr.s->l) { done.push_back(leaf_root[next_leaf++]); st.pop_back(); continue; }
                        if (fr.state == 0) { fr.state = 1; st.push_back(Frame{ fr.s->l.get(), 0, -1 }); continue; }
                        if (fr.state == 1) { fr.state = 2; st.push_back(Frame{ fr.s->r.get(), 0, -1 }); continue; }
                        const int r = done.back(); done.pop_back();
                        const int l = done.back(); done.pop_back();
                        done.push_back(T.add(l, r, -1));
                        st.pop_back();
                }
                F.tasks.assign(3 * (size_t)(F.n - 1), 0);
                if (emit_tasks(T, done.back(), F.n, F.tasks.data()) != F.n - 1) bad_count++;
                // msa->seq_distances (bisectingKmeans.c:244-255)
                if (seq_distances)
                        for (int i = 0; i < F.n; i++) {
                                float sum = 0.0f;
                                for (int j = 0; j < F.A; j++) sum += F.dm[(size_t)i * F.padded + j];
                                const float mean_dist = sum / (float)F.A;
                                seq_distances[F.first + i] = mean_dist / (float)flen[i];
                        }
        });
        if (bad_count) return ka_fail_message((me + ": internal error (task count)").c_str());

        // ---- one task list: leaves carry their global index, internal nodes are numseq + the task's place in the list ----
        int t0 = 0;
        for (const Fam& F : fams) {
                if (F.n < 2) continue;
                for (int t = 0; t < F.n - 1; t++)
                        for (int k = 0; k < 3; k++) {
                                const int x = F.tasks[3 * (size_t)t + k];
                                tasks_abc[3 * (size_t)(t0 + t) + k] = x < F.n ? F.first + x : numseq + t0 + (x - F.n);
                        }
                t0 += F.n - 1;
        }
        if (n_tasks_out) *n_tasks_out = t0;
        return KA_OK;
}

// Tests only: the host's split2 on one set from one seed, with what it went through.  dm[numrows][32]; lists: sl at 0, sr at n.
extern "C" int ka_debug_kmeans_host(const float* dm, int numrows, const int* samples, int n, int seed_pick,
                                    float* score, int* counts, int* lists, float* mind, float* wmean, int* counters)
{
        if (!dm || !samples || numrows < 1 || n < 1 || seed_pick < 0 || seed_pick >= n || !score || !counts || !lists || !mind || !wmean || !counters)
                return ka_fail_message("ka_debug_kmeans_host: bad arguments");
        for (int i = 0; i < n; i++)
                if (samples[i] < 0 || samples[i] >= numrows) return ka_fail_message("ka_debug_kmeans_host: sample out of range");
        try {
                Split res;
                SplitTrace tr;
                split2<true>(dm, KA_MAX_ANCHORS, std::vector<int>(samples, samples + n), KA_MAX_ANCHORS, seed_pick, res, &tr);
                *score = res.score;
                counts[0] = (int)res.sl.size(); counts[1] = (int)res.sr.size();
                std::copy(res.sl.begin(), res.sl.end(), lists);
                std::copy(res.sr.begin(), res.sr.end(), lists + n);
                std::copy(tr.mind.begin(), tr.mind.end(), mind);
                std::copy(tr.w.begin(), tr.w.end(), wmean);
                counters[0] = tr.iterations; counters[1] = tr.parity_total; counters[2] = tr.parity_last; counters[3] = tr.degenerate ? 1 : 0;
        } catch (const std::exception& e) {
                return ka_fail_message((std::string("ka_debug_kmeans_host: ") + e.what()).c_str());
        }
        return KA_OK;
}

// upgma()'s bookkeeping (bisectingKmeans.c:996-1047) for a merge sequence found on the device: merge k joins the
// current subtrees of slots a < b into slot a; the last merge's slot holds the root.  Library-internal.
__attribute__((visibility("hidden"))) int ka_tasks_from_merges(int numseq, const int* merges_ab, int* tasks_abc)
{
        Tree T;
        std::vector<int> slot(numseq);
        for (int i = 0; i < numseq; i++) slot[i] = T.add(-1, -1, i);
        int top = slot[0];
        for (int k = 0; k < numseq - 1; k++) {
                const int a = merges_ab[2 * k], b = merges_ab[2 * k + 1];
                if (a < 0 || b < 0 || a >= numseq || b >= numseq || a == b || slot[a] < 0 || slot[b] < 0)
                        return ka_fail_message("realignment tree: inconsistent merge sequence");
                slot[a] = T.add(slot[a], slot[b], -1);
                slot[b] = -1;
                top = slot[a];
        }
        return emit_tasks(T, top, numseq, tasks_abc) == numseq - 1 ? KA_OK : ka_fail_message("realignment tree: internal error (task count)");
}

// The distance source of the product: the two batches run on the device (ka_bpm.hip).
namespace {
struct DeviceDist { ka_ctx* ctx; const uint8_t* codes; const int* off; const int* lens; int numseq; double ms; };
int device_dist(void* user, int npairs, const int* ia, const int* ib, int* out)
{
        DeviceDist* D = (DeviceDist*)user;
        if (ka_bpm_batch(D->ctx, D->codes, D->off, D->lens, D->numseq, ia, ib, npairs, out)) return 1;
        D->ms += ka_pairwise_kernel_ms(D->ctx);
        return 0;
}
thread_local double g_last_dist_ms = 0.0;
}  // namespace
// device ms of the distance batches of this thread's last ka_guide_forest (library-internal: ka_run_encoded_batch's stage times)
__attribute__((visibility("hidden"))) double ka_guide_last_dist_ms(void) { return g_last_dist_ms; }

extern "C" int ka_guide_tree(ka_ctx* ctx, int numseq, const uint8_t* codes, const int* off, const int* lens,
                             int n_threads, const float* dm_scale, int* tasks_abc, float* seq_distances)
{
        if (!ctx || !codes || !off) return ka_fail_message("ka_guide_tree: bad arguments");
        DeviceDist D{ ctx, codes, off, lens, numseq, 0.0 };
        g_km = KmDevice();
        g_km.on = ka_ctx_device_stream(ctx, &g_km.device, &g_km.stream) == 0;
        const int rc = ka_guide_tree_from(numseq, lens, device_dist, &D, n_threads, dm_scale, tasks_abc, seq_distances);
        g_km = KmDevice();
        return rc;
}

extern "C" int ka_guide_forest(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* codes, const int* off, const int* lens,
                               int n_threads, const float* dm_scale, int* tasks_abc, int* n_tasks_out, float* seq_distances)
{
        if (!ctx || !codes || !off || !fam_first || n_fam < 1) return ka_fail_message("ka_guide_forest: bad arguments");
        DeviceDist D{ ctx, codes, off, lens, fam_first[n_fam], 0.0 };
        g_km = KmDevice();
        g_km.on = ka_ctx_device_stream(ctx, &g_km.device, &g_km.stream) == 0;
        const int rc = ka_guide_forest_from(n_fam, fam_first, lens, device_dist, &D, n_threads, dm_scale, tasks_abc, n_tasks_out, seq_distances);
        g_last_dist_ms = D.ms;
        g_km = KmDevice();
        return rc;
}

// Tests only: one level of the device bisection through the function ka_kmeans_device calls for it (ka_kmeans.hip: km_level).
extern "C" int ka_debug_kmeans_level(ka_ctx* ctx, const float* dm, int numrows, const int* samples, int n_samples,
                                     const int* sets_start_n, int n_sets, int force_big,
                                     float* score, int* counts, int* lists, float* mind, float* wmean, int* winner, int* big_out)
{
        int device = 0;
        hipStream_t stream = nullptr;
        if (!ctx || ka_ctx_device_stream(ctx, &device, &stream)) return ka_fail_message("ka_debug_kmeans_level: bad context");
        if (!score || !counts || !lists || !mind || !wmean || !winner) return ka_fail_message("ka_debug_kmeans_level: bad arguments");
        try {
                std::string why;
                if (ka_kmeans_debug_level(device, stream, dm, numrows, samples, n_samples, sets_start_n, n_sets, force_big,
                                          score, counts, lists, mind, wmean, winner, big_out, why)) return ka_fail_message(why.c_str());
        } catch (const std::exception& e) {
                return ka_fail_message((std::string("ka_debug_kmeans_level: ") + e.what()).c_str());
        }
        return KA_OK;
}
