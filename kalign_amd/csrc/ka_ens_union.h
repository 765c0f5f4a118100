// ka_ens_union.h -- the sequential part of the ensemble consensus stage, for both of its handles (ka_ens.cpp: one family;
// ka_ens_fam.cpp: a batch of families, one family per host thread at a time): build_consensus' greedy union of the
// candidate pairs (consensus_msa.c:372-562), the column order after it (topo_sort, consensus_msa.c:255-370) and the fill.
// Library-internal and host-only: the standard library and nothing of HIP.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

struct Uf {
        // union by rank with path halving; per-set member lists; sequence sets as bitmasks, kept for sets of two or
        // more residues only (a singleton's set is the bit of its own sequence)
        std::vector<int> parent, rnk, elemSeq, head, next, tail, maskOf;
        std::vector<uint64_t> pool;
        std::vector<int> freeSlots;
        int mw = 1;
        std::vector<long long> visited;
        long long visit = 0;
        long long truncations = 0;
        const std::vector<int>* offs = nullptr;
        const std::vector<int>* lens = nullptr;

        void init(const std::vector<int>& o, const std::vector<int>& l, int T)
        {
                offs = &o; lens = &l;
                const int N = (int)l.size();
                mw = (N + 63) / 64;
                parent.resize(T); rnk.assign(T, 0); elemSeq.resize(T); head.resize(T); next.assign(T, -1); tail.resize(T);
                maskOf.assign(T, -1); visited.assign(T, 0);
                pool.clear(); freeSlots.clear(); visit = 0; truncations = 0;
                for (int e = 0; e < T; e++) { parent[e] = e; head[e] = e; tail[e] = e; }
                for (int s = 0; s < N; s++)
                        for (int p = 0; p < l[s]; p++) elemSeq[o[s] + p] = s;
        }
        int find(int x)
        {
                while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
                return x;
        }
        bool hasSeq(int root, int s) const
        {
                const int m = maskOf[root];
                if (m < 0) return elemSeq[root] == s;
                return pool[(size_t)m * mw + s / 64] >> (s % 64) & 1u;
        }
        bool share(int a, int b) const
        {
                const int ma = maskOf[a], mb = maskOf[b];
                if (ma < 0) return hasSeq(b, elemSeq[a]);
                if (mb < 0) return hasSeq(a, elemSeq[b]);
                for (int w = 0; w < mw; w++)
                        if (pool[(size_t)ma * mw + w] & pool[(size_t)mb * mw + w]) return true;
                return false;
        }
        int slot()
        {
                if (!freeSlots.empty()) { const int s = freeSlots.back(); freeSlots.pop_back(); std::fill_n(&pool[(size_t)s * mw], mw, 0); return s; }
                pool.resize(pool.size() + mw, 0);
                return (int)(pool.size() / mw) - 1;
        }
        // is `target` reachable from `start` through the column DAG?  Queue of 4096 sets, full = not queued (still marked)
        bool reaches(int start, int target)
        {
                int queue[4096];
                int qh = 0, qt = 0;
                if (start == target) return true;
                visit++;
                queue[qt++] = start;
                visited[start] = visit;
                while (qh < qt) {
                        const int cur = queue[qh++];
                        for (int e = head[cur]; e >= 0; e = next[e]) {
                                const int s = elemSeq[e];
                                if (e - (*offs)[s] + 1 >= (*lens)[s]) continue;
                                const int r = find(e + 1);
                                if (r == target) return true;
                                if (r != cur && visited[r] != visit) {
                                        visited[r] = visit;
                                        if (qt < 4096) queue[qt++] = r;
                                        else truncations++;
                                }
                        }
                }
                return false;
        }
        void join(int a, int b)
        {
                const int ra = find(a), rb = find(b);
                if (ra == rb) return;
                if (share(ra, rb)) return;
                if (reaches(ra, rb)) return;
                if (reaches(rb, ra)) return;
                int keep, gone;
                if (rnk[ra] < rnk[rb]) { keep = rb; gone = ra; }
                else { keep = ra; gone = rb; if (rnk[ra] == rnk[rb]) rnk[ra]++; }
                parent[gone] = keep;
                if (maskOf[keep] < 0) {
                        const int s = slot();
                        maskOf[keep] = s;
                        pool[(size_t)s * mw + elemSeq[keep] / 64] |= 1ull << (elemSeq[keep] % 64);
                }
                uint64_t* km = &pool[(size_t)maskOf[keep] * mw];
                if (maskOf[gone] < 0) km[elemSeq[gone] / 64] |= 1ull << (elemSeq[gone] % 64);
                else {
                        const uint64_t* gm = &pool[(size_t)maskOf[gone] * mw];
                        for (int w = 0; w < mw; w++) km[w] |= gm[w];
                        freeSlots.push_back(maskOf[gone]);
                        maskOf[gone] = -1;
                }
                if (head[gone] >= 0) {
                        if (head[keep] < 0) { head[keep] = head[gone]; tail[keep] = tail[gone]; }
                        else { next[tail[keep]] = head[gone]; tail[keep] = tail[gone]; }
                }
                head[gone] = -1;
        }
};

// DFS topological sort of the columns, back edges skipped; returns order[position] = column
inline std::vector<int> topo_order(const std::vector<int>& colId, const std::vector<int>& offs, const std::vector<int>& lens, int nCols)
{
        std::vector<std::vector<int>> adj(nCols);
        for (size_t s = 0; s < lens.size(); s++)
                for (int p = 0; p + 1 < lens[s]; p++) {
                        const int ca = colId[offs[s] + p], cb = colId[offs[s] + p + 1];
                        if (ca == cb) continue;
                        std::vector<int>& l = adj[ca];
                        if (std::find(l.begin(), l.end(), cb) == l.end()) l.push_back(cb);
                }
        std::vector<int> out(nCols), state(nCols, 0), stack;
        stack.reserve(2 * (size_t)nCols);
        int at = nCols - 1;
        for (int start = 0; start < nCols; start++) {
                if (state[start]) continue;
                stack.push_back(start); stack.push_back(0);
                state[start] = 1;
                while (!stack.empty()) {
                        const int edge = stack.back(); stack.pop_back();
                        const int node = stack.back(); stack.pop_back();
                        bool pushed = false;
                        for (int e = edge; e < (int)adj[node].size(); e++) {
                                const int nx = adj[node][e];
                                if (state[nx] == 0) {
                                        stack.push_back(node); stack.push_back(e + 1);
                                        stack.push_back(nx); stack.push_back(0);
                                        state[nx] = 1;
                                        pushed = true;
                                        break;
                                }
                        }
                        if (!pushed) { state[node] = 2; out[at--] = node; }
                }
        }
        return out;
}

// the columns of a finished union numbered by the first residue (flat order) of each set, ordered, and filled with the
// letters: rows = N x *nColsOut bytes, '-' where a sequence has no residue
inline void ka_ens_fill(Uf& uf, const std::vector<int>& offs, const std::vector<int>& lens, int T, const uint8_t* letters, std::vector<uint8_t>& rows,
                        int* nColsOut)
{
        const int N = (int)lens.size();
        std::vector<int> rootCol(T, -1), colId(T);
        int nCols = 0;
        for (int e = 0; e < T; e++) {
                const int r = uf.find(e);
                if (rootCol[r] < 0) rootCol[r] = nCols++;
                colId[e] = rootCol[r];
        }
        const std::vector<int> order = topo_order(colId, offs, lens, nCols);
        std::vector<int> pos(nCols);
        for (int p = 0; p < nCols; p++) pos[order[p]] = p;
        rows.assign((size_t)N * nCols, '-');
        for (int s = 0; s < N; s++)
                for (int p = 0; p < lens[s]; p++) rows[(size_t)s * nCols + pos[colId[offs[s] + p]]] = letters[offs[s] + p];
        *nColsOut = nCols;
}

// one family from its candidates to its consensus rows: the union over the candidates (pairs of residue numbers flat inside
// the family, 2 ints each, in the reference's order; handed over in one piece or level by level), then the columns.  Touches
// nothing but itself and its arguments: families run on any thread in any order.  Not to be moved once init has run (the
// union points at the lengths).
struct KaEnsFamilyUnion {
        std::vector<int> l, o;
        int T = 0;
        Uf uf;
        double ms = 0.0;                                         // (the caller's account of the time spent on this family)

        void init(int N, const int* lens)
        {
                l.assign(lens, lens + N);
                o.assign(N + 1, 0);
                for (int s = 0; s < N; s++) o[s + 1] = o[s] + l[s];
                T = o[N];
                uf.init(o, l, T);
        }
        void join(const int* cand, long long n)
        {
                for (long long x = 0; x < n; x++) uf.join(cand[2 * x], cand[2 * x + 1]);
        }
        void finish(const uint8_t* letters, std::vector<uint8_t>& rows, int* nColsOut) { ka_ens_fill(uf, o, l, T, letters, rows, nColsOut); }
};

// fn(f) for f0 <= f < f1 on up to n_threads threads (the caller's among them), each taking the next family when it is free.
// fn writes only what belongs to f, so the outcome does not depend on n_threads.  Returns false when an fn threw.
template <class Fn>
inline bool ka_ens_deal(int f0, int f1, int n_threads, Fn fn)
{
        std::atomic<int> next(f0);
        std::atomic<bool> ok(true);
        auto work = [&]() {
                for (;;) {
                        const int f = next.fetch_add(1);
                        if (f >= f1) return;
                        try { fn(f); } catch (...) { ok = false; }
                }
        };
        const int extra = std::min(n_threads, f1 - f0) - 1;
        std::vector<std::thread> th;
        for (int t = 0; t < extra; t++) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
        return ok;
}
