// ka_ens.cpp -- host side of the ensemble consensus stage (kalign_ensemble's tail, lib/src/ensemble.c:341-): the ka_ens
// handle of the C ABI, and the one part of the stage that stays sequential -- build_consensus' greedy union of the
// candidate pairs (consensus_msa.c:372-562) and the column order after it.
//
// The device (ka_ens.hip) turns the members' rows into position maps and walks (i, j, ri) for scores, confidences and
// candidates.  The candidates come one support level at a time, highest first, in the reference's order inside a level
// (i, j, ri, rj ascending; the stable counting sort of consensus_msa.c:438-459 over the table order).  A level is cut
// into chunks of whole rows i; while the greedy replays chunk c from pinned memory, the device writes chunk c + 1.
//
// The greedy is order-dependent in two ways and is replayed candidate by candidate:
//   * a merge is refused when the two sets share a sequence, or when either set reaches the other in the column DAG
//     (an edge from a residue's set to the set of the next residue of the same sequence);
//   * that reachability search is a breadth-first search with a queue of 4096 sets that silently stops queueing when
//     full (dag_reachable, consensus_msa.c:121-160) -- its answer depends on the order of the sets' member lists,
//     i.e. on the merge history.  The lists are concatenated as the reference does (the absorbed set's list after the
//     surviving root's), the root chosen by rank as it does.
// The same chunked hand-over carries the members' POAR table to a file (ka_ens_table_write; poar_table_write,
// poar.c:203-252), and a handle opened from such a file (ka_ens_open_table; poar_table_read, poar.c:254-325) reads its
// support and its candidates from the table on the device (ka_poar.hip) and feeds the same greedy.
// The columns are numbered by the first residue (flat order) of each set, ordered by a DFS topological sort that skips
// back edges (topo_sort, consensus_msa.c:255-370) and filled with the caller's letters.
#include "ka_ctx.h"
#include "ka_ens.h"
#include "ka_ens_union.h"     // Uf, topo_order, ka_ens_fill: shared with ka_ens_fam.cpp
#include "ka_msa.h"

int ka_ctx_device_stream(ka_ctx* c, int* device, hipStream_t* stream);    // (library-internal: ka_api.cpp)

namespace {

double ms_since(std::chrono::steady_clock::time_point t0)
{
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

} // namespace

struct ka_ens {
        ka_ctx* ctx = nullptr;
        int device = 0;
        hipStream_t stream = nullptr;
        KaSeqSet q;
        int R = 0;
        std::vector<int> W;
        std::vector<DevBuf<uint8_t>> rows;            // member k's rows, N x W[k]
        DevBuf<int> dCol, dColX, dCnt, dSup, dNp;
        DevBuf<int16_t> dRes, dResX;
        DevBuf<uint8_t> dRowsX;
        DevBuf<long long> dPairOff, dRowTot, dRowBase[2];
        DevBuf<unsigned long long> dScore;
        DevBuf<int2> dOut[2];
        DevBuf<float> dConf, dColConf;
        int2* pinned[2] = { nullptr, nullptr };
        long long pinnedCap = 0, chunkCap = 0;
        hipEvent_t ready[2] = { nullptr, nullptr }, wBeg[2] = { nullptr, nullptr }, wEnd[2] = { nullptr, nullptr }, ev0 = nullptr, ev1 = nullptr;
        bool mapsFresh = false;
        long long generation = 0;
        // a handle opened from a POAR table: no members, the table on the device
        bool fromTable = false;
        long long tabEntries = 0;                     // of the loaded table; of the members' table once counted (tabCountGen)
        long long tabCountGen = -1;
        DevBuf<long long> dPairStart;                 // [N * (N - 1) / 2 + 1]
        DevBuf<uint2> dEnt;
        double tab[KA_ENS_TABLE_STATS] = {};          // ka_ens_table_stats
        // the last consensus (a caller with a too narrow buffer asks again)
        long long cacheGen = -1;
        int cacheMin = -1, cacheW = 0;
        std::vector<uint8_t> cacheRows;
        std::vector<uint8_t> cacheLetters;
        // measurements of the last call of each kind
        double st[KA_ENS_STATS] = {};
        long long levelCount[KA_ENS_MAX_RUNS + 1] = {};
        double levelMs[KA_ENS_MAX_RUNS + 1] = {};

        ~ka_ens()
        {
                for (int b = 0; b < 2; b++) {
                        if (pinned[b]) (void)hipHostFree(pinned[b]);
                        if (ready[b]) (void)hipEventDestroy(ready[b]);
                        if (wBeg[b]) (void)hipEventDestroy(wBeg[b]);
                        if (wEnd[b]) (void)hipEventDestroy(wEnd[b]);
                        dOut[b].release(); dRowBase[b].release();
                }
                if (ev0) (void)hipEventDestroy(ev0);
                if (ev1) (void)hipEventDestroy(ev1);
                for (auto& r : rows) r.release();
                q.release();
                dCol.release(); dColX.release(); dCnt.release(); dSup.release(); dNp.release();
                dRes.release(); dResX.release(); dRowsX.release(); dPairOff.release(); dRowTot.release(); dScore.release();
                dConf.release(); dColConf.release(); dPairStart.release(); dEnt.release();
        }

        float evMs() { float m = 0.0f; (void)hipEventElapsedTime(&m, ev0, ev1); return m; }

        int ensure_maps()
        {
                if (mapsFresh || fromTable) return KA_OK;
                for (int k = 0; k < R; k++)
                        if (W[k] <= 0) return fail("ka_ens: member " + std::to_string(k) + " not added (all n_runs members are needed)");
                const int N = q.N, T = q.T;
                long long resTot = 0;
                for (int k = 0; k < R; k++) resTot += (long long)N * W[k];
                if (dCol.alloc((size_t)R * T) || dRes.alloc((size_t)resTot)) return fail("ka_ens: out of device memory (maps)");
                HIPCHK(hipEventRecord(ev0, stream));
                long long o = 0;
                for (int k = 0; k < R; k++) {
                        ka_msa_launch_maps(rows[k].p, W[k], W[k], W[k], q, dCol.p + (long long)k * T, dRes.p + o, stream);
                        o += (long long)N * W[k];
                }
                HIPCHK(hipGetLastError());
                HIPCHK(hipEventRecord(ev1, stream));
                HIPCHK(hipEventSynchronize(ev1));
                st[0] = evMs();
                mapsFresh = true;
                return KA_OK;
        }

        KaEnsArgs args()
        {
                KaEnsArgs a{};
                a.offs = q.dOffs; a.lens = q.dLens; a.N = q.N; a.R = R; a.T = q.T; a.maxlen = q.maxlen;
                a.col = dCol.p; a.res = dRes.p;
                long long o = 0;
                for (int k = 0; k < R; k++) { a.resOff[k] = o; a.W[k] = W[k]; o += (long long)q.N * W[k]; }
                a.i0 = 0; a.i1 = q.N;
                // the member columns of sequence i in LDS when they fit next to the three per-residue arrays (64 KiB)
                a.colInLds = (long long)(3 + R) * q.maxlen * 4 <= 65536;
                a.pairStart = dPairStart.p; a.ent = dEnt.p;
                return a;
        }

        // an alignment X's maps in dColX / dResX
        int maps_x(const uint8_t* r, long long stride, int alnlen, KaEnsArgs& a)
        {
                if (dRowsX.alloc((size_t)q.N * alnlen) || dColX.alloc((size_t)std::max(q.T, 1)) || dResX.alloc((size_t)q.N * alnlen))
                        return fail("ka_ens: out of device memory");
                if (ka_msa_upload_rows(q, dRowsX.p, r, stride, alnlen, stream)) return KA_FAIL;
                ka_msa_launch_maps(dRowsX.p, alnlen, alnlen, alnlen, q, dColX.p, dResX.p, stream);
                a.colX = dColX.p; a.resX = dResX.p; a.Wx = alnlen;
                return KA_OK;
        }

        // SCORE / CONF / the candidates' COUNT / WRITE from the handle's source of support
        void launch_support(int mode, const KaEnsArgs& a)
        {
                if (!fromTable) ka_ens_launch_walk(mode, a, stream);
                else if (mode == KA_ENS_SCORE || mode == KA_ENS_CONF) ka_poar_launch_lookup(mode, a, stream);
                else ka_poar_launch_level(mode, a, stream);
        }

        template <class Count>
        int count_rows(KaEnsArgs& a, int b0, int b1, Count count, std::vector<long long>& rowTot, std::vector<int>* pairCnt, double* countMs);
        template <class Count, class Write, class Consume>
        int stream_rows(KaEnsArgs a, Count count, Write write, Consume consume, std::vector<int>* pairCnt, double* countMs, double* writeMs, double* waitMs, double* chunks, long long* total);
        int consensus(int minSup, const uint8_t* letters);
        struct Sink;
        int table_count(long long* entries);
        int table_emit(Sink* sink);
        int load_table(const uint8_t* image, long long nBytes);
        struct TabRef { const long long* pairStart; const uint2* ent; long long entries; };
        int pair_starts(int b0, int b1, const std::vector<long long>& rowTot, long long* run, long long* pairStart);
        int table_on_device(DevBuf<long long>& ps, DevBuf<uint2>& ent, TabRef* t);
        template <class Launch>
        int derive_table(const char* who, KaEnsArgs a, Launch launch);
};

// rows i per count pass: the pair counts and offsets of a block are rows x N entries
static int ens_count_block(int N) { return std::max(1, std::min(N, (int)((1ll << 24) / std::max(N, 1)))); }

// count(a) over rows b0 .. b1 and the row scan: a.cnt and dPairOff on the device, the rows' totals (and, when asked for, the
// pairs' counts) on the host
template <class Count>
int ka_ens::count_rows(KaEnsArgs& a, int b0, int b1, Count count, std::vector<long long>& rowTot, std::vector<int>* pairCnt, double* countMs)
{
        const int N = q.N, rb = ens_count_block(N);
        if (dCnt.alloc((size_t)rb * N) || dPairOff.alloc((size_t)rb * N) || dRowTot.alloc((size_t)rb)) return fail("ka_ens: out of device memory (counts)");
        rowTot.resize(rb);
        a.i0 = b0; a.i1 = b1; a.cnt = dCnt.p;
        HIPCHK(hipEventRecord(ev0, stream));
        HIPCHK(hipMemsetAsync(dCnt.p, 0, sizeof(int) * (size_t)(b1 - b0) * N, stream));
        count(a);
        ka_ens_launch_row_scan(dCnt.p, N, dPairOff.p, dRowTot.p, b1 - b0, stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev1, stream));
        HIPCHK(hipMemcpyAsync(rowTot.data(), dRowTot.p, sizeof(long long) * (b1 - b0), hipMemcpyDeviceToHost, stream));
        if (pairCnt) {
                pairCnt->resize((size_t)(b1 - b0) * N);
                HIPCHK(hipMemcpyAsync(pairCnt->data(), dCnt.p, sizeof(int) * (size_t)(b1 - b0) * N, hipMemcpyDeviceToHost, stream));
        }
        HIPCHK(hipStreamSynchronize(stream));
        *countMs += evMs();
        return KA_OK;
}

// One pass over all rows i of a per-pair list (candidates of a level, or table entries): count(a) fills a.cnt for rows
// a.i0 .. a.i1, the rows are scanned and cut into chunks of whole rows of at most chunkCap items (a longer row is a chunk of
// its own), write(w) puts chunk c + 1 into the other device buffer while consume(i0, i1, b0, items, n) takes chunk c from
// pinned memory (b0: first row of the count block, for pairCnt -- the block's counts on the host, when asked for).
template <class Count, class Write, class Consume>
int ka_ens::stream_rows(KaEnsArgs a, Count count, Write write, Consume consume, std::vector<int>* pairCnt, double* countMs, double* writeMs, double* waitMs, double* chunks, long long* total)
{
        using clk = std::chrono::steady_clock;
        const int N = q.N;
        const int rb = ens_count_block(N);
        std::vector<long long> rowTot;
        std::vector<long long> rowBase[2];
        for (int b0 = 0; b0 < N; b0 += rb) {
                const int b1 = std::min(N, b0 + rb);
                if (count_rows(a, b0, b1, count, rowTot, pairCnt, countMs)) return KA_FAIL;
                // chunks of whole rows, each at most chunkCap items (a longer row is a chunk of its own)
                std::vector<int> cut{ b0 };
                std::vector<long long> tot;
                long long run = 0, biggest = 0;
                for (int i = b0; i < b1; i++) {
                        const long long t = rowTot[i - b0];
                        *total += t;
                        if (run > 0 && run + t > chunkCap) { cut.push_back(i); tot.push_back(run); biggest = std::max(biggest, run); run = 0; }
                        run += t;
                }
                cut.push_back(b1); tot.push_back(run); biggest = std::max(biggest, run);
                if (biggest > pinnedCap) {
                        HIPCHK(hipStreamSynchronize(stream));
                        for (int q = 0; q < 2; q++) {
                                if (pinned[q]) (void)hipHostFree(pinned[q]);
                                pinned[q] = nullptr;
                                HIPCHK(hipHostMalloc((void**)&pinned[q], sizeof(int2) * (size_t)biggest));
                                if (dOut[q].alloc((size_t)biggest)) return fail("ka_ens: out of device memory (candidates)");
                        }
                        pinnedCap = biggest;
                }
                const int nChunks = (int)tot.size();
                auto enqueue = [&](int c) -> int {
                        const int q = c & 1;
                        if (tot[c] == 0) return KA_OK;
                        rowBase[q].assign(cut[c + 1] - cut[c], 0);
                        // rowBase[i - i0] + pairOff[(i - i0) * N + j]: the write pass indexes both by the launch's i0
                        long long o = 0;
                        for (int i = cut[c]; i < cut[c + 1]; i++) { rowBase[q][i - cut[c]] = o; o += rowTot[i - b0]; }
                        if (dRowBase[q].alloc(rowBase[q].size())) return fail("ka_ens: out of device memory");
                        HIPCHK(hipMemcpyAsync(dRowBase[q].p, rowBase[q].data(), sizeof(long long) * rowBase[q].size(), hipMemcpyHostToDevice, stream));
                        KaEnsArgs w = a;
                        w.i0 = cut[c]; w.i1 = cut[c + 1];
                        w.pairOff = dPairOff.p + (long long)(cut[c] - b0) * N;
                        w.rowBase = dRowBase[q].p; w.out = dOut[q].p; w.entOut = reinterpret_cast<uint2*>(dOut[q].p);
                        HIPCHK(hipEventRecord(wBeg[q], stream));
                        write(w);
                        HIPCHK(hipGetLastError());
                        HIPCHK(hipEventRecord(wEnd[q], stream));
                        HIPCHK(hipMemcpyAsync(pinned[q], dOut[q].p, sizeof(int2) * (size_t)tot[c], hipMemcpyDeviceToHost, stream));
                        HIPCHK(hipEventRecord(ready[q], stream));
                        return KA_OK;
                };
                if (enqueue(0)) return KA_FAIL;
                for (int c = 0; c < nChunks; c++) {
                        if (c + 1 < nChunks && enqueue(c + 1)) return KA_FAIL;
                        if (tot[c] == 0) {
                                if (consume(cut[c], cut[c + 1], b0, (const int2*)nullptr, 0LL)) return KA_FAIL;
                                continue;
                        }
                        const auto t0 = clk::now();
                        HIPCHK(hipEventSynchronize(ready[c & 1]));
                        *waitMs += ms_since(t0);
                        float wms = 0.0f;
                        (void)hipEventElapsedTime(&wms, wBeg[c & 1], wEnd[c & 1]);
                        *writeMs += wms;
                        if (consume(cut[c], cut[c + 1], b0, pinned[c & 1], tot[c])) return KA_FAIL;
                        *chunks += 1;
                }
        }
        return KA_OK;
}

int ka_ens::consensus(int minSup, const uint8_t* letters)
{
        using clk = std::chrono::steady_clock;
        const int T = q.T;
        const std::vector<int>& lens = q.lens;
        const std::vector<int>& offs = q.offs;
        st[2] = st[3] = st[4] = st[5] = st[7] = st[8] = st[9] = 0.0;
        std::fill_n(levelCount, KA_ENS_MAX_RUNS + 1, 0LL);
        std::fill_n(levelMs, KA_ENS_MAX_RUNS + 1, 0.0);
        if (ensure_maps()) return KA_FAIL;
        KaEnsArgs a = args();
        Uf uf;
        uf.init(offs, lens, T);
        for (int L = R; L >= std::max(minSup, 1); L--) {
                a.level = L;
                double cms = 0.0, wms = 0.0;
                const int rc = stream_rows(a, [&](const KaEnsArgs& x) { launch_support(KA_ENS_COUNT, x); }, [&](const KaEnsArgs& x) { launch_support(KA_ENS_WRITE, x); },
                                           [&](int, int, int, const int2* p, long long n) {
                                                   const auto t1 = clk::now();
                                                   for (long long x = 0; x < n; x++) uf.join(p[x].x, p[x].y);
                                                   st[4] += ms_since(t1);
                                                   return KA_OK;
                                           }, nullptr, &cms, &wms, &st[7], &st[8], &levelCount[L]);
                if (rc) return rc;
                st[2] += cms; st[3] += wms; levelMs[L] += cms + wms;
        }
        st[9] = (double)uf.truncations;
        // columns numbered by first residue, ordered, filled
        const auto tt = clk::now();
        int nCols = 0;
        ka_ens_fill(uf, offs, lens, T, letters, cacheRows, &nCols);
        st[5] = ms_since(tt);
        cacheW = nCols; cacheMin = minSup; cacheGen = generation;
        cacheLetters.assign(letters, letters + T);
        return KA_OK;
}

// where the file's bytes go: a file, or memory of `cap` bytes
struct ka_ens::Sink {
        FILE* fp = nullptr;
        uint8_t* mem = nullptr;
        long long cap = 0, at = 0;
        int put(const void* p, size_t n)
        {
                if (fp) {
                        if (std::fwrite(p, 1, n, fp) != n) return fail("ka_ens_table_write: writing the file failed");
                } else {
                        if (at + (long long)n > cap) return fail("ka_ens_table_image: the buffer is smaller than the table (ka_ens_table_size)");
                        std::memcpy(mem + at, p, n);
                }
                at += (long long)n;
                return KA_OK;
        }
};

// the number of entries of the table: count passes only, kept until a member changes
int ka_ens::table_count(long long* entries)
{
        if (fromTable) { *entries = tabEntries; return KA_OK; }
        if (ensure_maps()) return KA_FAIL;
        if (tabCountGen != generation) {
                KaEnsArgs a = args();
                const int N = q.N, rb = ens_count_block(N);
                std::vector<long long> rowTot;
                long long total = 0;
                double ms = 0.0;
                for (int b0 = 0; b0 < N; b0 += rb) {
                        const int b1 = std::min(N, b0 + rb);
                        if (count_rows(a, b0, b1, [&](const KaEnsArgs& x) { ka_poar_launch_table(KA_ENS_COUNT, x, stream); }, rowTot, nullptr, &ms)) return KA_FAIL;
                        for (int i = b0; i < b1; i++) total += rowTot[i - b0];
                }
                tabEntries = total;
                tabCountGen = generation;
        }
        *entries = tabEntries;
        return KA_OK;
}

// poar_table_write's bytes (poar.c:216-252) into the sink: the header, then per pair its count and its entries.  The
// device emits counts and entries apart (the count word would leave the entries 4-byte aligned); they meet here.
int ka_ens::table_emit(Sink* sink)
{
        using clk = std::chrono::steady_clock;
        if (ensure_maps()) return KA_FAIL;
        KaEnsArgs a = args();
        a.level = 0;
        const int N = q.N;
        std::fill_n(tab, KA_ENS_TABLE_STATS, 0.0);
        const uint32_t head[4] = { 0x524F4150u, 1u, (uint32_t)N, (uint32_t)R };
        if (sink->put(head, sizeof head)) return KA_FAIL;
        std::vector<int> cnt;
        long long total = 0;
        const int rc = stream_rows(a,
                [&](const KaEnsArgs& x) { if (fromTable) ka_poar_launch_level(KA_ENS_COUNT, x, stream); else ka_poar_launch_table(KA_ENS_COUNT, x, stream); },
                [&](const KaEnsArgs& x) { if (fromTable) ka_poar_launch_level(KA_ENS_WRITE, x, stream); else ka_poar_launch_table(KA_ENS_WRITE, x, stream); },
                [&](int i0, int i1, int b0, const int2* p, long long) {
                        const auto t0 = clk::now();
                        long long o = 0;
                        for (int i = i0; i < i1; i++)
                                for (int j = i + 1; j < N; j++) {
                                        const uint32_t c = (uint32_t)cnt[(size_t)(i - b0) * N + j];
                                        if (sink->put(&c, 4)) return KA_FAIL;
                                        if (c && sink->put(p + o, 8 * (size_t)c)) return KA_FAIL;
                                        o += c;
                                }
                        tab[2] += ms_since(t0);
                        return KA_OK;
                }, &cnt, &tab[0], &tab[1], &tab[5], &tab[4], &total);
        if (rc) return rc;
        tab[3] = (double)total;
        if (!fromTable) { tabEntries = total; tabCountGen = generation; }
        if (sink->at != 16 + 4 * ((long long)N * (N - 1) / 2) + 8 * total) return fail("ka_ens: the table's bytes do not add up to its counts");
        return KA_OK;
}

// the checked table of a file image onto the device: first entry of every pair, entries
int ka_ens::load_table(const uint8_t* image, long long nBytes)
{
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<long long> ps;
        int runs = 0;
        if (ka_poar_parse(image, nBytes, q.N, q.lens.data(), &runs, &tabEntries, &ps)) return KA_FAIL;
        R = runs;
        W.assign(R, 0);
        fromTable = true;
        std::vector<uint2> ent((size_t)tabEntries);
        long long at = 16;
        for (size_t p = 0; p + 1 < ps.size(); p++) {
                const long long c = ps[p + 1] - ps[p];
                if (c) std::memcpy(&ent[(size_t)ps[p]], image + at + 4, 8 * (size_t)c);
                at += 4 + 8 * c;
        }
        if (dPairStart.alloc(ps.size()) || dEnt.alloc((size_t)std::max(tabEntries, 1LL))) return fail("ka_ens_open_table: out of device memory (the table)");
        HIPCHK(hipMemcpyAsync(dPairStart.p, ps.data(), sizeof(long long) * ps.size(), hipMemcpyHostToDevice, stream));
        if (tabEntries) HIPCHK(hipMemcpyAsync(dEnt.p, ent.data(), sizeof(uint2) * (size_t)tabEntries, hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
        tab[2] = ms_since(t0);
        tab[3] = (double)tabEntries;
        return KA_OK;
}

// rows b0 .. b1 as count_rows left them (dPairOff, rowTot): the first entry of each of their pairs into pairStart, where *run
// entries lie before row b0; the rows' own first entries stay in dRowBase[0], and *run moves on to row b1
int ka_ens::pair_starts(int b0, int b1, const std::vector<long long>& rowTot, long long* run, long long* pairStart)
{
        std::vector<long long> base((size_t)(b1 - b0));
        for (int i = b0; i < b1; i++) { base[i - b0] = *run; *run += rowTot[i - b0]; }
        if (dRowBase[0].alloc(base.size())) return fail("ka_ens: out of device memory");
        HIPCHK(hipMemcpyAsync(dRowBase[0].p, base.data(), sizeof(long long) * base.size(), hipMemcpyHostToDevice, stream));
        ka_poar_launch_pair_start(dPairOff.p, dRowBase[0].p, b0, b1, q.N, pairStart, stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        return KA_OK;
}

// the handle's table where a kernel can read it: a table-backed handle's own; the members' table built into ps / ent in full
// (the table passes of table_emit, without the chunked hand-over to the host)
int ka_ens::table_on_device(DevBuf<long long>& ps, DevBuf<uint2>& ent, TabRef* t)
{
        if (fromTable) { *t = TabRef{ dPairStart.p, dEnt.p, tabEntries }; return KA_OK; }
        long long total = 0;
        if (table_count(&total)) return KA_FAIL;
        const int N = q.N, rb = ens_count_block(N);
        const long long nPairs = (long long)N * (N - 1) / 2;
        if (ps.alloc((size_t)nPairs + 1) || ent.alloc((size_t)std::max(total, 1LL)))
                return fail("ka_ens: out of device memory (the table of a member-backed operand, " + std::to_string(total) + " entries)");
        KaEnsArgs a = args();
        std::vector<long long> rowTot;
        long long run = 0;
        double ms = 0.0;
        for (int b0 = 0; b0 < N; b0 += rb) {
                const int b1 = std::min(N, b0 + rb);
                if (count_rows(a, b0, b1, [&](const KaEnsArgs& x) { ka_poar_launch_table(KA_ENS_COUNT, x, stream); }, rowTot, nullptr, &ms)) return KA_FAIL;
                if (pair_starts(b0, b1, rowTot, &run, ps.p)) return KA_FAIL;
                KaEnsArgs w = a;
                w.pairOff = dPairOff.p; w.rowBase = dRowBase[0].p; w.entOut = ent.p;
                ka_poar_launch_table(KA_ENS_WRITE, w, stream);
                HIPCHK(hipGetLastError());
        }
        if (run != total) return fail("ka_ens: the table's counts changed between two passes");
        HIPCHK(hipMemcpyAsync(ps.p + nPairs, &run, sizeof(long long), hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
        *t = TabRef{ ps.p, ent.p, total };
        return KA_OK;
}

// this handle's table from launch(COUNT / WRITE, args): a is ready but for what the passes fill in.  COUNT gives every pair its
// size, so the pairs' first entries are known before the one WRITE pass, which reads them (a.outStart) as the table's reader will.
template <class Launch>
int ka_ens::derive_table(const char* who, KaEnsArgs a, Launch launch)
{
        const int N = q.N, rb = ens_count_block(N);
        const long long nPairs = (long long)N * (N - 1) / 2;
        if (dPairStart.alloc((size_t)nPairs + 1)) return fail(std::string(who) + ": out of device memory (the table)");
        std::fill_n(tab, KA_ENS_TABLE_STATS, 0.0);
        std::vector<long long> rowTot;
        long long run = 0;
        for (int b0 = 0; b0 < N; b0 += rb) {
                const int b1 = std::min(N, b0 + rb);
                if (count_rows(a, b0, b1, [&](const KaEnsArgs& x) { launch(KA_ENS_COUNT, x); }, rowTot, nullptr, &tab[0])) return KA_FAIL;
                if (pair_starts(b0, b1, rowTot, &run, dPairStart.p)) return KA_FAIL;
        }
        if (dEnt.alloc((size_t)std::max(run, 1LL))) return fail(std::string(who) + ": out of device memory (the table, " + std::to_string(run) + " entries)");
        HIPCHK(hipMemcpyAsync(dPairStart.p + nPairs, &run, sizeof(long long), hipMemcpyHostToDevice, stream));
        a.i0 = 0; a.i1 = N;
        a.outStart = dPairStart.p; a.entOut = dEnt.p;
        HIPCHK(hipEventRecord(ev0, stream));
        launch(KA_ENS_WRITE, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev1, stream));
        HIPCHK(hipStreamSynchronize(stream));
        tab[1] = evMs();
        tabEntries = run;
        tab[3] = (double)run;
        return KA_OK;
}

// a handle on ctx's device and stream for these sequences, without a source of support yet
static int ens_new(const char* who, ka_ctx* ctx, int numseq, const int* lens, std::unique_ptr<ka_ens>& e)
{
        e.reset(new ka_ens);
        e->ctx = ctx;
        if (ka_ctx_device_stream(ctx, &e->device, &e->stream)) return fail(std::string(who) + ": bad context");
        HIPCHK(hipSetDevice(e->device));
        if (e->q.init(who, numseq, lens, KA_ENS_MAX_RES,
                      "residue indices must stay below 4096 (the reference's POAR key ri << 20 | rj aliases beyond)"))
                return KA_FAIL;
        const char* cc = std::getenv("KA_ENS_CHUNK");                    // candidates per chunk (tests force many chunks)
        e->chunkCap = cc && std::atoll(cc) > 0 ? std::atoll(cc) : (1ll << 22);
        if (e->dScore.alloc(1)) return fail(std::string(who) + ": out of device memory");
        for (int b = 0; b < 2; b++) {
                HIPCHK(hipEventCreateWithFlags(&e->ready[b], hipEventDisableTiming));
                HIPCHK(hipEventCreate(&e->wBeg[b]));
                HIPCHK(hipEventCreate(&e->wEnd[b]));
        }
        HIPCHK(hipEventCreate(&e->ev0));
        HIPCHK(hipEventCreate(&e->ev1));
        return KA_OK;
}

extern "C" int ka_ens_create(ka_ctx* ctx, int numseq, const int* lens, int n_runs, ka_ens** out)
{
        if (!ctx || !out || numseq < 1 || !lens) return fail("ka_ens_create: bad arguments");
        if (n_runs < 1 || n_runs > KA_ENS_MAX_RUNS)
                return fail("ka_ens_create: n_runs " + std::to_string(n_runs) + " outside 1.." + std::to_string(KA_ENS_MAX_RUNS) + " (one bit per member in the reference's POAR table)");
        *out = nullptr;
        std::unique_ptr<ka_ens> e;
        if (ens_new("ka_ens_create", ctx, numseq, lens, e)) return KA_FAIL;
        e->R = n_runs;
        e->W.assign(n_runs, 0);
        e->rows.resize(n_runs);
        *out = e.release();
        return KA_OK;
}

extern "C" void ka_ens_destroy(ka_ens* e)
{
        if (!e) return;
        (void)hipSetDevice(e->device);
        (void)hipStreamSynchronize(e->stream);
        delete e;
}

extern "C" int ka_ens_add_member(ka_ens* e, int k, const uint8_t* rows, long long row_stride, int alnlen)
{
        if (e && e->fromTable) return fail("ka_ens_add_member: this handle was opened from a POAR table and takes no members");
        if (!e || k < 0 || k >= e->R) return fail("ka_ens_add_member: bad arguments");
        if (ka_msa_check_rows("ka_ens_add_member", e->q, rows, row_stride, alnlen)) return KA_FAIL;
        HIPCHK(hipSetDevice(e->device));
        if (e->rows[k].alloc((size_t)e->q.N * alnlen)) return fail("ka_ens_add_member: out of device memory");
        if (ka_msa_upload_rows(e->q, e->rows[k].p, rows, row_stride, alnlen, e->stream)) return KA_FAIL;
        HIPCHK(hipStreamSynchronize(e->stream));
        e->W[k] = alnlen;
        e->mapsFresh = false;
        e->generation++;
        return KA_OK;
}

extern "C" int ka_ens_score_rows(ka_ens* e, const uint8_t* rows, long long row_stride, int alnlen, long long* sum_out, double* score_out)
{
        if (!e) return fail("ka_ens_score_rows: bad arguments");
        if (ka_msa_check_rows("ka_ens_score_rows", e->q, rows, row_stride, alnlen)) return KA_FAIL;
        HIPCHK(hipSetDevice(e->device));
        if (e->ensure_maps()) return KA_FAIL;
        KaEnsArgs a = e->args();
        HIPCHK(hipEventRecord(e->ev0, e->stream));
        if (e->maps_x(rows, row_stride, alnlen, a)) return KA_FAIL;
        HIPCHK(hipMemsetAsync(e->dScore.p, 0, sizeof(unsigned long long), e->stream));
        a.score = e->dScore.p;
        e->launch_support(KA_ENS_SCORE, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->ev1, e->stream));
        unsigned long long s = 0;
        HIPCHK(hipMemcpyAsync(&s, e->dScore.p, sizeof(s), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        e->st[1] = e->evMs();
        const long long S = (long long)s;
        if (sum_out) *sum_out = S;
        if (score_out) *score_out = (double)S / (e->R > 1 ? (double)(e->R - 1) : 1.0);
        return KA_OK;
}

extern "C" int ka_ens_consensus(ka_ens* e, int min_support, const uint8_t* letters, uint8_t* rows_out, long long row_stride, int* alnlen_out)
{
        if (!e || !letters || min_support < 1) return fail("ka_ens_consensus: bad arguments (min_support >= 1, letters)");
        HIPCHK(hipSetDevice(e->device));
        const bool cached = e->cacheGen == e->generation && e->cacheMin == min_support &&
                            std::equal(e->cacheLetters.begin(), e->cacheLetters.end(), letters) && (int)e->cacheLetters.size() == e->q.T;
        if (!cached && e->consensus(min_support, letters)) return KA_FAIL;
        if (alnlen_out) *alnlen_out = e->cacheW;
        if (!rows_out || row_stride < e->cacheW) return KA_ERR_ROWS_STRIDE;
        for (int s = 0; s < e->q.N; s++)
                std::memcpy(rows_out + (long long)s * row_stride, e->cacheRows.data() + (size_t)s * e->cacheW, e->cacheW);
        return KA_OK;
}

extern "C" int ka_ens_confidence(ka_ens* e, const uint8_t* rows, long long row_stride, int alnlen, float* res_conf_out, float* col_conf_out)
{
        if (!e || !res_conf_out || !col_conf_out) return fail("ka_ens_confidence: bad arguments");
        if (ka_msa_check_rows("ka_ens_confidence", e->q, rows, row_stride, alnlen)) return KA_FAIL;
        HIPCHK(hipSetDevice(e->device));
        if (e->ensure_maps()) return KA_FAIL;
        KaEnsArgs a = e->args();
        HIPCHK(hipEventRecord(e->ev0, e->stream));
        if (e->maps_x(rows, row_stride, alnlen, a)) return KA_FAIL;
        if (e->dSup.alloc((size_t)std::max(e->q.T, 1)) || e->dNp.alloc((size_t)std::max(e->q.T, 1)) ||
            e->dConf.alloc((size_t)e->q.N * alnlen) || e->dColConf.alloc((size_t)alnlen))
                return fail("ka_ens_confidence: out of device memory");
        HIPCHK(hipMemsetAsync(e->dSup.p, 0, sizeof(int) * (size_t)std::max(e->q.T, 1), e->stream));
        HIPCHK(hipMemsetAsync(e->dNp.p, 0, sizeof(int) * (size_t)std::max(e->q.T, 1), e->stream));
        a.supSum = e->dSup.p; a.nPair = e->dNp.p;
        e->launch_support(KA_ENS_CONF, a);
        ka_ens_launch_conf(a, e->dConf.p, e->dColConf.p, e->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->ev1, e->stream));
        HIPCHK(hipMemcpyAsync(res_conf_out, e->dConf.p, sizeof(float) * (size_t)e->q.N * alnlen, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(col_conf_out, e->dColConf.p, sizeof(float) * (size_t)alnlen, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        e->st[6] = e->evMs();
        return KA_OK;
}

extern "C" int ka_ens_stats(ka_ens* e, double* stats_out, long long* level_counts_out, double* level_ms_out)
{
        if (!e) return fail("ka_ens_stats: bad arguments");
        if (stats_out) std::copy_n(e->st, KA_ENS_STATS, stats_out);
        if (level_counts_out) std::copy_n(e->levelCount, KA_ENS_MAX_RUNS + 1, level_counts_out);
        if (level_ms_out) std::copy_n(e->levelMs, KA_ENS_MAX_RUNS + 1, level_ms_out);
        return KA_OK;
}

extern "C" int ka_ens_n_runs(ka_ens* e) { return e ? e->R : 0; }

extern "C" int ka_ens_table_size(ka_ens* e, long long* bytes_out, long long* entries_out)
{
        if (!e) return fail("ka_ens_table_size: bad arguments");
        HIPCHK(hipSetDevice(e->device));
        long long n = 0;
        if (e->table_count(&n)) return KA_FAIL;
        if (bytes_out) *bytes_out = 16 + 4 * ((long long)e->q.N * (e->q.N - 1) / 2) + 8 * n;
        if (entries_out) *entries_out = n;
        return KA_OK;
}

extern "C" int ka_ens_table_write(ka_ens* e, const char* path)
{
        if (!e || !path) return fail("ka_ens_table_write: bad arguments");
        HIPCHK(hipSetDevice(e->device));
        if (e->ensure_maps()) return KA_FAIL;
        ka_ens::Sink sink;
        sink.fp = std::fopen(path, "wb");
        if (!sink.fp) return fail(std::string("ka_ens_table_write: cannot open ") + path + " for writing");
        int rc = e->table_emit(&sink);
        if (std::fclose(sink.fp) != 0 && !rc) rc = fail(std::string("ka_ens_table_write: closing ") + path + " failed");
        if (rc) (void)std::remove(path);                                  // no truncated file is left behind
        return rc;
}

extern "C" int ka_ens_table_image(ka_ens* e, uint8_t* out, long long cap)
{
        if (!e || !out || cap < 0) return fail("ka_ens_table_image: bad arguments");
        HIPCHK(hipSetDevice(e->device));
        ka_ens::Sink sink;
        sink.mem = out; sink.cap = cap;
        return e->table_emit(&sink);
}

extern "C" int ka_ens_open_table_image(ka_ctx* ctx, int numseq, const int* lens, const uint8_t* image, long long n_bytes, ka_ens** out)
{
        if (!ctx || !out || numseq < 1 || !lens || !image) return fail("ka_ens_open_table: bad arguments");
        *out = nullptr;
        std::unique_ptr<ka_ens> e;
        if (ens_new("ka_ens_open_table", ctx, numseq, lens, e)) return KA_FAIL;
        if (e->load_table(image, n_bytes)) return KA_FAIL;
        *out = e.release();
        return KA_OK;
}

extern "C" int ka_ens_open_table(ka_ctx* ctx, int numseq, const int* lens, const char* path, ka_ens** out)
{
        if (!path) return fail("ka_ens_open_table: bad arguments");
        FILE* fp = std::fopen(path, "rb");
        if (!fp) return fail(std::string("ka_ens_open_table: cannot open ") + path + " for reading");
        std::vector<uint8_t> image;
        std::vector<uint8_t> block(1 << 20);
        size_t n;
        while ((n = std::fread(block.data(), 1, block.size(), fp)) > 0) image.insert(image.end(), block.begin(), block.begin() + n);
        const bool bad = std::ferror(fp) != 0;
        std::fclose(fp);
        if (bad) return fail(std::string("ka_ens_open_table: reading ") + path + " failed");
        const uint8_t none = 0;                                           // (an empty file: the reader says so)
        return ka_ens_open_table_image(ctx, numseq, lens, image.empty() ? &none : image.data(), (long long)image.size(), out);
}

// a table-backed handle of n_runs members for the sequences of `like`, its table still to come (derive_table)
static int ens_new_result(const char* who, const ka_ens* like, int n_runs, std::unique_ptr<ka_ens>& o)
{
        if (ens_new(who, like->ctx, like->q.N, like->q.lens.data(), o)) return KA_FAIL;
        o->R = n_runs;
        o->W.assign(n_runs, 0);
        o->fromTable = true;
        return KA_OK;
}

extern "C" int ka_ens_merge(ka_ens* a, ka_ens* b, ka_ens** out)
{
        const char* who = "ka_ens_merge";
        if (!a || !b || !out) return fail("ka_ens_merge: bad arguments (a NULL handle or a NULL out)");
        if (a->ctx != b->ctx) return fail("ka_ens_merge: the two handles belong to different contexts");
        if (a->q.N != b->q.N)
                return fail("ka_ens_merge: numseq " + std::to_string(a->q.N) + " in the first handle, " + std::to_string(b->q.N) + " in the second");
        for (int s = 0; s < a->q.N; s++)
                if (a->q.lens[s] != b->q.lens[s])
                        return fail("ka_ens_merge: sequence " + std::to_string(s) + " has " + std::to_string(a->q.lens[s]) + " residues in the first handle, " +
                                    std::to_string(b->q.lens[s]) + " in the second");
        if (a->R + b->R > KA_ENS_MAX_RUNS)
                return fail("ka_ens_merge: " + std::to_string(a->R) + " + " + std::to_string(b->R) + " members exceed " + std::to_string(KA_ENS_MAX_RUNS) +
                            " (one bit per member in the reference's POAR table)");
        HIPCHK(hipSetDevice(a->device));
        DevBuf<long long> psA, psB;
        DevBuf<uint2> entA, entB;
        ka_ens::TabRef ta{}, tb{};
        std::unique_ptr<ka_ens> o;
        int rc = a->table_on_device(psA, entA, &ta);
        if (!rc) rc = b->table_on_device(psB, entB, &tb);
        if (!rc) rc = ens_new_result(who, a, a->R + b->R, o);
        if (!rc) {
                KaEnsArgs x = o->args();
                x.pairStart = ta.pairStart; x.ent = ta.ent;
                x.pairStartB = tb.pairStart; x.entB = tb.ent;
                x.shift = a->R;
                hipStream_t s = o->stream;
                rc = o->derive_table(who, x, [s](int mode, const KaEnsArgs& y) { ka_poar_launch_merge(mode, y, s); });
        }
        psA.release(); psB.release(); entA.release(); entB.release();
        if (rc) return rc;
        *out = o.release();
        return KA_OK;
}

extern "C" int ka_ens_select(ka_ens* e, const int* members, int n, ka_ens** out)
{
        const char* who = "ka_ens_select";
        if (!e || !members || !out) return fail("ka_ens_select: bad arguments (a NULL handle, NULL members or a NULL out)");
        if (n < 1 || n > e->R) return fail("ka_ens_select: n = " + std::to_string(n) + " outside 1.." + std::to_string(e->R) + " (the handle's n_runs)");
        unsigned seen = 0;
        for (int t = 0; t < n; t++) {
                if (members[t] < 0 || members[t] >= e->R)
                        return fail("ka_ens_select: member index " + std::to_string(members[t]) + " out of range 0.." + std::to_string(e->R - 1));
                if (seen >> members[t] & 1u) return fail("ka_ens_select: member " + std::to_string(members[t]) + " given twice");
                seen |= 1u << members[t];
        }
        HIPCHK(hipSetDevice(e->device));
        DevBuf<long long> ps;
        DevBuf<uint2> ent;
        ka_ens::TabRef te{};
        std::unique_ptr<ka_ens> o;
        int rc = e->table_on_device(ps, ent, &te);
        if (!rc) rc = ens_new_result(who, e, n, o);
        if (!rc) {
                KaEnsArgs x = o->args();
                x.pairStart = te.pairStart; x.ent = te.ent;
                x.nSel = n;
                for (int t = 0; t < n; t++) x.sel[t] = (unsigned char)members[t];
                hipStream_t s = o->stream;
                rc = o->derive_table(who, x, [s](int mode, const KaEnsArgs& y) { ka_poar_launch_select(mode, y, s); });
        }
        ps.release(); ent.release();
        if (rc) return rc;
        *out = o.release();
        return KA_OK;
}

extern "C" int ka_ens_table_stats(ka_ens* e, double* out6)
{
        if (!e || !out6) return fail("ka_ens_table_stats: bad arguments");
        std::copy_n(e->tab, KA_ENS_TABLE_STATS, out6);
        return KA_OK;
}
