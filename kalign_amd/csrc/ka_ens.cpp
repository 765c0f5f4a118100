// ka_ens.cpp -- host side of the ensemble consensus stage (kalign_ensemble's tail, lib/src/ensemble.c:341-): KaEnsCore
// (ka_ens_core.h), the one host core of the stage, and over it the ka_ens handle of the C ABI -- a table of one family.
// (ka_ens_fam.cpp is the front for a batch of families.)
//
// The device (ka_ens.hip) turns the members' rows into position maps and walks (i, j, ri) for scores, confidences and
// candidates.  The candidates of every support level are counted in one pass over a block of rows and written one level
// at a time, highest first, in the reference's order inside a level (i, j, ri, rj ascending; the stable counting sort of
// consensus_msa.c:438-459 over the table order).  A level is cut into chunks (here: of whole rows i); while the host takes
// chunk c from pinned memory, the device writes chunk c + 1.
//
// The one part of the stage that stays sequential is build_consensus' greedy union of the candidate pairs
// (consensus_msa.c:372-562) and the column order after it (ka_ens_union.h); this front runs it on the calling thread.
// The greedy is order-dependent in two ways and is replayed candidate by candidate:
//   * a merge is refused when the two sets share a sequence, or when either set reaches the other in the column DAG
//     (an edge from a residue's set to the set of the next residue of the same sequence);
//   * that reachability search is a breadth-first search with a queue of 4096 sets that silently stops queueing when
//     full (dag_reachable, consensus_msa.c:121-160) -- its answer depends on the order of the sets' member lists,
//     i.e. on the merge history.  The lists are concatenated as the reference does (the absorbed set's list after the
//     surviving root's), the root chosen by rank as it does.
// The same count-a-block and hand-over sequences carry the members' POAR table to a file (ka_ens_table_write;
// poar_table_write, poar.c:203-252), and a handle opened from such a file (ka_ens_open_table; poar_table_read,
// poar.c:254-325) reads its support and its candidates from the table on the device (ka_poar.hip) and feeds the same greedy.
// The columns are numbered by the first residue (flat order) of each set, ordered by a DFS topological sort that skips
// back edges (topo_sort, consensus_msa.c:255-370) and filled with the caller's letters.
#include "ka_ens_core.h"
#include "ka_ens_union.h"     // Uf, topo_order, ka_ens_fill: shared with ka_ens_fam.cpp

// ---------------------------------------------------------------- the core ----------------------------------------------------------------

KaEnsCore::~KaEnsCore()
{
        for (int b = 0; b < 2; b++) {
                if (pinned[b]) (void)hipHostFree(pinned[b]);
                if (ready[b]) (void)hipEventDestroy(ready[b]);
                if (wBeg[b]) (void)hipEventDestroy(wBeg[b]);
                if (wEnd[b]) (void)hipEventDestroy(wEnd[b]);
        }
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
}

void KaEnsCore::close()
{
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
}

int KaEnsCore::create(const char* who, ka_ctx* ctx, int n_fam, const int* fam_first, const int* l, int n_runs, int rowPadBytes)
{
        const std::string me(who);
        if (ka_ctx_device_stream(ctx, &device, &stream)) return fail(me + ": bad context");
        F = n_fam; S = fam_first[n_fam]; R = n_runs; rowPad = rowPadBytes;
        famFirst.assign(fam_first, fam_first + F + 1);
        lens.assign(l, l + S);
        offs.resize(S + 1);
        int t = 0;
        for (int s = 0; s < S; s++) { offs[s] = t; t += l[s]; }
        offs[S] = T = t;
        fams.resize(F);
        blkFirst.resize(F + 1);
        long long blocks = 0;
        for (int f = 0; f < F; f++) {
                KaEnsFam& d = fams[f];
                d = KaEnsFam{};
                d.firstSeq = fam_first[f]; d.firstRes = offs[fam_first[f]];
                d.N = fam_first[f + 1] - fam_first[f];
                for (int s = 0; s < d.N; s++) d.maxlen = std::max(d.maxlen, l[d.firstSeq + s]);
                d.nJC = (d.N + KA_ENS_JCHUNK - 1) / KA_ENS_JCHUNK;
                // the member columns of sequence i in LDS when they fit next to the three per-residue arrays (64 KiB)
                d.colInLds = (long long)(3 + R) * d.maxlen * 4 <= 65536;
                d.minSup = 1;
                ldsX = std::max(ldsX, (size_t)(3 * d.maxlen + (d.colInLds ? R * d.maxlen : 0)) * sizeof(int));
                ldsCand = std::max(ldsCand, (size_t)(d.colInLds ? R * d.maxlen : 0) * sizeof(int));
                d.cntFirst = E;
                E += (long long)d.N * d.N;
                blkFirst[f] = (int)blocks;
                blocks += (long long)d.N * d.nJC;
                if (blocks > INT32_MAX) return fail(me + ": more than 2^31 - 1 workgroups in a walk over the batch");
        }
        blkFirst[F] = nBlocks = (int)blocks;
        added.assign(R, 0);
        memW.assign((size_t)R * F, 0);
        memCell.assign((size_t)R * (F + 1), 0);
        memRowOff.assign((size_t)R * F, 0);
        dRows.resize(R);
        const char* cc = std::getenv("KA_ENS_CHUNK");                    // candidates per chunk (tests force many chunks)
        chunkCap = cc && std::atoll(cc) > 0 ? std::atoll(cc) : (1ll << 22);
        const char* cr = std::getenv("KA_ENS_COUNT_ROWS");               // rows per count block of ka_ens (tests force many blocks)
        countRows = cr && std::atoi(cr) > 0 ? std::atoi(cr) : 0;
        HIPCHK(hipSetDevice(device));
        for (int b = 0; b < 2; b++) {
                HIPCHK(hipEventCreateWithFlags(&ready[b], hipEventDisableTiming));
                HIPCHK(hipEventCreate(&wBeg[b]));
                HIPCHK(hipEventCreate(&wEnd[b]));
        }
        HIPCHK(hipEventCreate(&ev0));
        HIPCHK(hipEventCreate(&ev1));
        if (dFams.alloc(F) || dFirstSeq.alloc(F + 1) || dBlkFirst.alloc(F + 1) || dOffs.alloc(S + 1) || dLens.alloc(S) ||
            dMemW.alloc(memW.size()) || dMemCell.alloc(memCell.size()) || dMemRowOff.alloc(memRowOff.size()) ||
            dXTab.alloc((size_t)3 * F + 2) || dXRowOff.alloc(F) || dScore.alloc((size_t)R * F) ||
            dSup.alloc((size_t)std::max(t, 1)) || dNp.alloc((size_t)std::max(t, 1)))
                return fail(me + ": out of device memory");
        HIPCHK(hipMemcpyAsync(dFams.p, fams.data(), sizeof(KaEnsFam) * F, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dFirstSeq.p, famFirst.data(), sizeof(int) * (F + 1), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dBlkFirst.p, blkFirst.data(), sizeof(int) * (F + 1), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dOffs.p, offs.data(), sizeof(int) * (S + 1), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dLens.p, lens.data(), sizeof(int) * S, hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return KA_OK;
}

KaEnsFamArgs KaEnsCore::args() const
{
        KaEnsFamArgs a{};
        a.nFam = F; a.S = S; a.T = T; a.R = R;
        a.rows = S; a.E = E;
        a.fams = dFams.p; a.firstSeq = dFirstSeq.p; a.blkFirst = dBlkFirst.p; a.offs = dOffs.p; a.lens = dLens.p;
        a.col = dCol.p; a.res = dRes.p; a.memCell = dMemCell.p; a.memW = dMemW.p;
        std::copy_n(resBase, KA_ENS_MAX_RUNS, a.resBase);
        return a;
}

int KaEnsCore::member_fits(const char* who, int k, const int* alnlens) const
{
        long long c = 0;
        for (int f = 0; f < F; f++) c += (long long)fams[f].N * alnlens[f];
        if (c > INT32_MAX) return fail(std::string(who) + ": more than 2^31 - 1 cells in the maps of member " + std::to_string(k));
        return KA_OK;
}

// (the member's entries of the three tables go to the device here, stream-ordered, from vectors that outlive the copies: the
// maps launches of ensure_maps then follow no upload)
int KaEnsCore::member_added(int k, const int* alnlens)
{
        long long ro = 0, c = 0;
        for (int f = 0; f < F; f++) {
                memW[(size_t)k * F + f] = alnlens[f];
                memRowOff[(size_t)k * F + f] = ro;
                memCell[(size_t)k * (F + 1) + f] = (int)c;
                ro += (long long)fams[f].N * (alnlens[f] + rowPad);
                c += (long long)fams[f].N * alnlens[f];
        }
        memCell[(size_t)k * (F + 1) + F] = (int)c;
        HIPCHK(hipMemcpyAsync(dMemW.p + (size_t)k * F, &memW[(size_t)k * F], sizeof(int) * F, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dMemCell.p + (size_t)k * (F + 1), &memCell[(size_t)k * (F + 1)], sizeof(int) * (F + 1), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dMemRowOff.p + (size_t)k * F, &memRowOff[(size_t)k * F], sizeof(long long) * F, hipMemcpyHostToDevice, stream));
        added[k] = 1;
        mapsFresh = false;
        return KA_OK;
}

int KaEnsCore::ensure_maps(const char* who)
{
        if (mapsFresh) return KA_OK;
        for (int k = 0; k < R; k++)
                if (!added[k]) return fail(std::string(who) + ": member " + std::to_string(k) + " not added (all n_runs members are needed)");
        long long o = 0;
        for (int k = 0; k < R; k++) { resBase[k] = o; o += memCell[(size_t)k * (F + 1) + F]; }
        if (dCol.alloc((size_t)R * std::max(T, 1)) || dRes.alloc((size_t)o)) return fail(std::string(who) + ": out of device memory (maps)");
        HIPCHK(hipEventRecord(ev0, stream));
        const KaMsaFamRows t{ F, S, dFirstSeq.p, dOffs.p, dLens.p };
        for (int k = 0; k < R; k++) {
                ka_msa_launch_maps_fam(t, dRows[k].p, dMemRowOff.p + (size_t)k * F, dMemW.p + (size_t)k * F, dMemCell.p + (size_t)k * (F + 1), rowPad,
                                   dCol.p + (long long)k * T, dRes.p + resBase[k], stream);
                nLaunch++;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev1, stream));
        HIPCHK(hipEventSynchronize(ev1));
        nSync++;
        mapsMs = evMs();
        mapsFresh = true;
        return KA_OK;
}

int KaEnsCore::maps_x(const char* who, const int* alnlens, const KaEnsUpload& upload, KaEnsFamArgs& a, int* cells, int* cols)
{
        // xW [F] | xCell [F + 1] | xCol [F + 1]; they and the rows' offsets outlive their copies: no wait on the host here
        std::vector<int>& tab = xTab;
        std::vector<long long>& rowOff = xRowOff;
        tab.resize((size_t)3 * F + 2);
        rowOff.resize(F);
        int* xW = tab.data();
        int* xCell = xW + F;
        int* xCol = xCell + F + 1;
        long long ro = 0, c = 0;
        int w = 0;
        for (int f = 0; f < F; f++) {
                const int W = std::max(alnlens[f], 0);
                xW[f] = W; xCell[f] = (int)c; xCol[f] = w; rowOff[f] = ro;
                c += (long long)fams[f].N * W;
                w += W;
                if (W > 0) ro += (long long)fams[f].N * (W + rowPad);
                if (c > INT32_MAX) return fail(std::string(who) + ": more than 2^31 - 1 cells in the alignment's maps");
        }
        xCell[F] = (int)c; xCol[F] = w;
        if (dRowsX.alloc((size_t)std::max(ro, 1LL)) || dColX.alloc((size_t)std::max(T, 1)) || dResX.alloc((size_t)std::max(c, 1LL)))
                return fail(std::string(xWho ? xWho : who) + ": out of device memory");
        if (upload(dRowsX.p, stream)) return KA_FAIL;
        HIPCHK(hipMemcpyAsync(dXTab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dXRowOff.p, rowOff.data(), sizeof(long long) * F, hipMemcpyHostToDevice, stream));
        a.colX = dColX.p; a.resX = dResX.p; a.xW = dXTab.p; a.xCell = dXTab.p + F; a.xCol = dXTab.p + 2 * F + 1;
        ka_msa_launch_maps_fam(KaMsaFamRows{ F, S, dFirstSeq.p, dOffs.p, dLens.p }, dRowsX.p, dXRowOff.p, a.xW, a.xCell, rowPad, dColX.p, dResX.p, stream);
        nLaunch++;
        *cells = (int)c; *cols = w;
        return KA_OK;
}

// dScore[0 .. n) to the caller: sums, and score_alignment_poar's doubles
int KaEnsCore::scores_back(long long* sums_out, double* scores_out, int n)
{
        std::vector<unsigned long long> s((size_t)n);
        HIPCHK(hipMemcpyAsync(s.data(), dScore.p, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        nSync++;
        scoreMs = evMs();
        for (int x = 0; x < n; x++) {
                const long long v = (long long)s[x];
                if (sums_out) sums_out[x] = v;
                if (scores_out) scores_out[x] = (double)v / (R > 1 ? (double)(R - 1) : 1.0);
        }
        return KA_OK;
}

int KaEnsCore::score_x(const char* who, const int* alnlens, const KaEnsUpload& upload, const KaEnsSupport* other, long long* sums_out, double* scores_out)
{
        KaEnsFamArgs a = args();
        int cells = 0, cols = 0;
        HIPCHK(hipEventRecord(ev0, stream));
        if (maps_x(who, alnlens, upload, a, &cells, &cols)) return KA_FAIL;
        HIPCHK(hipMemsetAsync(dScore.p, 0, sizeof(unsigned long long) * (size_t)F, stream));
        a.score = dScore.p;
        if (other) (*other)(a);
        else ka_ens_launch_walk(KA_ENS_SCORE, a, nBlocks, ldsX, stream);
        nLaunch++;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev1, stream));
        return scores_back(sums_out, scores_out, F);
}

int KaEnsCore::score_members(long long* sums_out, double* scores_out)
{
        HIPCHK(hipEventRecord(ev0, stream));
        HIPCHK(hipMemsetAsync(dScore.p, 0, sizeof(unsigned long long) * (size_t)R * F, stream));
        for (int k = 0; k < R; k++) {
                // member k as the alignment X: its maps are the walk's tables already
                KaEnsFamArgs a = args();
                a.colX = dCol.p + (long long)k * T; a.resX = dRes.p + resBase[k];
                a.xW = dMemW.p + (size_t)k * F; a.xCell = dMemCell.p + (size_t)k * (F + 1);
                a.score = dScore.p + (size_t)k * F;
                ka_ens_launch_walk(KA_ENS_SCORE, a, nBlocks, ldsX, stream);
                nLaunch++;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev1, stream));
        return scores_back(sums_out, scores_out, R * F);
}

int KaEnsCore::confidence(const char* who, const int* alnlens, const KaEnsUpload& upload, const KaEnsSupport* other, float* res_conf_out, float* col_conf_out)
{
        KaEnsFamArgs a = args();
        int cells = 0, cols = 0;
        HIPCHK(hipEventRecord(ev0, stream));
        if (maps_x(who, alnlens, upload, a, &cells, &cols)) return KA_FAIL;
        if (dConf.alloc((size_t)cells) || dColConf.alloc((size_t)cols)) return fail(std::string(who) + ": out of device memory");
        const size_t T1 = (size_t)std::max(T, 1);
        HIPCHK(hipMemsetAsync(dSup.p, 0, sizeof(int) * T1, stream));
        HIPCHK(hipMemsetAsync(dNp.p, 0, sizeof(int) * T1, stream));
        a.supSum = dSup.p; a.nPair = dNp.p;
        if (other) (*other)(a);
        else ka_ens_launch_walk(KA_ENS_CONF, a, nBlocks, ldsX, stream);
        ka_ens_launch_conf(a, cells, cols, dConf.p, dColConf.p, stream);
        nLaunch += 3;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev1, stream));
        HIPCHK(hipMemcpyAsync(res_conf_out, dConf.p, sizeof(float) * (size_t)cells, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(col_conf_out, dColConf.p, sizeof(float) * (size_t)cols, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        nSync++;
        confMs = evMs();
        return KA_OK;
}

int KaEnsCore::count_block(const char* who, KaEnsFamArgs& a, int nLev, const std::function<void(const KaEnsFamArgs&)>& count, std::vector<long long>& rowTot,
                           std::vector<int>* pairCnt, double* ms)
{
        const long long ents = (long long)std::max(nLev, 0) * a.E, rows = (long long)std::max(nLev, 0) * a.rows;
        if (ents > INT32_MAX) return fail(std::string(who) + ": more than 2^31 - 1 (level, i, j) counters in the batch");
        const int nRows = (int)rows;
        if (dCnt.alloc((size_t)std::max(ents, 1LL)) || dPairOff.alloc((size_t)std::max(ents, 1LL)) || dRowTot.alloc((size_t)std::max(nRows, 1)))
                return fail(std::string(who) + ": out of device memory (counts)");
        a.cnt = dCnt.p; a.pairOff = dPairOff.p;
        rowTot.assign((size_t)nRows, 0);
        HIPCHK(hipEventRecord(ev0, stream));
        HIPCHK(hipMemsetAsync(dCnt.p, 0, sizeof(int) * (size_t)std::max(ents, 1LL), stream));
        if (nLev > 0) {
                count(a);
                ka_ens_launch_row_scan(a, nRows, dPairOff.p, dRowTot.p, stream);
                nLaunch += 2;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev1, stream));
        if (nRows) HIPCHK(hipMemcpyAsync(rowTot.data(), dRowTot.p, sizeof(long long) * nRows, hipMemcpyDeviceToHost, stream));
        if (pairCnt) {
                pairCnt->resize((size_t)ents);
                if (ents) HIPCHK(hipMemcpyAsync(pairCnt->data(), dCnt.p, sizeof(int) * (size_t)ents, hipMemcpyDeviceToHost, stream));
        }
        HIPCHK(hipStreamSynchronize(stream));
        nSync++;
        *ms += evMs();
        return KA_OK;
}

int KaEnsCore::put_row_base(const char* oom, const std::vector<long long>& rowBase)
{
        if (rowBase.empty()) return KA_OK;
        if (dRowBase.alloc(rowBase.size())) return fail(oom);
        HIPCHK(hipMemcpyAsync(dRowBase.p, rowBase.data(), sizeof(long long) * rowBase.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));                    // (rowBase is read until here)
        nSync++;
        return KA_OK;
}

int KaEnsCore::hand_over(const char* who, const std::vector<KaEnsChunk>& chunks, const std::function<void(const KaEnsChunk&, int2* out)>& write,
                         const std::function<int(const KaEnsChunk&, const int2* items)>& consume, double* writeMs, double* waitMs, double* nChunks)
{
        long long biggest = 0;
        for (const KaEnsChunk& c : chunks) biggest = std::max(biggest, c.total);
        if (biggest > pinnedCap) {                               // (nothing is in flight: every earlier chunk has been consumed)
                for (int q = 0; q < 2; q++) {
                        if (pinned[q]) (void)hipHostFree(pinned[q]);
                        pinned[q] = nullptr;
                        pinnedCap = 0;
                        HIPCHK(hipHostMalloc((void**)&pinned[q], sizeof(int2) * (size_t)biggest));
                        if (dOut[q].alloc((size_t)biggest)) return fail(std::string(who) + ": out of device memory (candidates)");
                }
                pinnedCap = biggest;
        }
        const int n = (int)chunks.size();
        auto enqueue = [&](int c) -> int {
                const int q = c & 1;
                if (chunks[c].total == 0) return KA_OK;
                HIPCHK(hipEventRecord(wBeg[q], stream));
                write(chunks[c], dOut[q].p);
                nLaunch++;
                HIPCHK(hipGetLastError());
                HIPCHK(hipEventRecord(wEnd[q], stream));
                HIPCHK(hipMemcpyAsync(pinned[q], dOut[q].p, sizeof(int2) * (size_t)chunks[c].total, hipMemcpyDeviceToHost, stream));
                HIPCHK(hipEventRecord(ready[q], stream));
                return KA_OK;
        };
        if (n && enqueue(0)) return KA_FAIL;
        for (int c = 0; c < n; c++) {
                if (c + 1 < n && enqueue(c + 1)) return KA_FAIL;
                if (chunks[c].total == 0) {
                        if (consume(chunks[c], nullptr)) return KA_FAIL;
                        continue;
                }
                const auto t0 = std::chrono::steady_clock::now();
                HIPCHK(hipEventSynchronize(ready[c & 1]));
                nSync++;
                *waitMs += ka_ens_ms_since(t0);
                float wms = 0.0f;
                (void)hipEventElapsedTime(&wms, wBeg[c & 1], wEnd[c & 1]);
                *writeMs += wms;
                *nChunks += 1;
                if (consume(chunks[c], pinned[c & 1])) return KA_FAIL;
        }
        return KA_OK;
}

// ---------------------------------------------------------------- the one-family front ----------------------------------------------------------------

struct ka_ens {
        ka_ctx* ctx = nullptr;
        KaEnsCore core;                               // a table of one family: F = 1, rows alnlen bytes apart
        KaSeqSet q;                                   // (host side only: the checks of the caller's rows)
        int R = 0;
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

        // the family's tables once n_runs is known
        int open(const char* who, int n_runs)
        {
                const int first[2] = { 0, q.N };
                R = n_runs;
                core.xWho = "ka_ens";
                return core.create(who, ctx, 1, first, q.lens.data(), n_runs, 0);
        }

        int ensure_maps()
        {
                if (fromTable) return KA_OK;
                const int rc = core.ensure_maps("ka_ens");
                st[0] = core.mapsMs;
                return rc;
        }

        // the table passes' view of the same memory (ka_poar.hip); the members' maps are valid after ensure_maps
        KaEnsArgs args() const
        {
                KaEnsArgs a{};
                a.offs = core.dOffs.p; a.lens = core.dLens.p; a.N = q.N; a.R = R; a.T = q.T; a.maxlen = q.maxlen;
                a.col = core.dCol.p; a.res = core.dRes.p;
                for (int k = 0; k < R; k++) { a.resOff[k] = core.resBase[k]; a.W[k] = core.memW[k]; }
                a.i0 = 0; a.i1 = q.N;
                a.colInLds = core.fams[0].colInLds;
                a.pairStart = dPairStart.p; a.ent = dEnt.p;
                return a;
        }

        // SCORE / CONF of a table-backed handle: the X maps and outputs of the core's call, support looked up in the table
        KaEnsSupport lookup(int mode, int alnlen)
        {
                return [this, mode, alnlen](const KaEnsFamArgs& f) {
                        KaEnsArgs a = args();
                        a.colX = f.colX; a.resX = f.resX; a.Wx = alnlen;
                        a.score = f.score; a.supSum = f.supSum; a.nPair = f.nPair;
                        ka_poar_launch_lookup(mode, a, core.stream);
                };
        }

        KaEnsUpload upload(const uint8_t* rows, long long stride, int alnlen)
        {
                return [=](uint8_t* dst, hipStream_t s) { return alnlen > 0 ? ka_msa_upload_rows(q, dst, rows, stride, alnlen, s) : KA_OK; };
        }

        // rows i per count block: the pair counts and offsets of a block are rows x N entries per level
        int count_rows() const { return core.countRows ? std::min(core.countRows, q.N) : std::max(1, std::min(q.N, (int)((1ll << 24) / std::max(q.N, 1)))); }
        // a count table of rows b0 .. b1
        KaEnsFamArgs block_args(int b0, int b1) const
        {
                KaEnsFamArgs f = core.args();
                f.row0 = b0; f.rows = b1 - b0; f.cnt0 = (long long)b0 * q.N; f.E = (long long)(b1 - b0) * q.N;
                f.blk0 = b0 * core.fams[0].nJC;
                return f;
        }
        void cut_rows(int level, int b0, int b1, const long long* tot, long long* rowBase, std::vector<KaEnsChunk>& out, long long* total) const;
        typedef std::function<void(const KaEnsArgs&)> Pass;
        int count_table_block(const KaEnsArgs& a, int b0, int b1, const Pass& count, std::vector<long long>& rowTot, std::vector<int>* pairCnt, double* countMs);
        typedef std::function<int(int i0, int i1, int b0, const int2* items, long long n)> Consume;
        int stream_rows(const KaEnsArgs& a, const Pass& count, const Pass& write, const Consume& consume, std::vector<int>* pairCnt, double* countMs, double* writeMs, double* waitMs, double* chunks, long long* total);
        int consensus(int minSup, const uint8_t* letters);
        struct Sink;
        int table_count(long long* entries);
        int table_emit(Sink* sink);
        int load_table(const uint8_t* image, long long nBytes);
        struct TabRef { const long long* pairStart; const uint2* ent; long long entries; };
        int pair_starts(int b0, int b1, const std::vector<long long>& rowTot, long long* run, long long* pairStart);
        int table_on_device(DevBuf<long long>& ps, DevBuf<uint2>& ent, TabRef* t);
        int derive_table(const char* who, KaEnsArgs a, const std::function<void(int, const KaEnsArgs&)>& launch);
};

// One level's rows b0 .. b1 with tot[i - b0] items each, cut into chunks of whole rows of at most chunkCap items (a longer row
// is a chunk of its own; the last chunk may be empty); rowBase[i - b0]: the row's first slot in its chunk
void ka_ens::cut_rows(int level, int b0, int b1, const long long* tot, long long* rowBase, std::vector<KaEnsChunk>& out, long long* total) const
{
        const int nJC = core.fams[0].nJC;
        int c0 = b0;
        long long run = 0;
        for (int i = b0; i < b1; i++) {
                const long long t = tot[i - b0];
                *total += t;
                if (run > 0 && run + t > core.chunkCap) { out.push_back(KaEnsChunk{ level, c0, i, c0 * nJC, (i - c0) * nJC, run }); c0 = i; run = 0; }
                rowBase[i - b0] = run;
                run += t;
        }
        out.push_back(KaEnsChunk{ level, c0, b1, c0 * nJC, (b1 - c0) * nJC, run });
}

// count(x) of a table pass over rows b0 .. b1 as one level of the count table: x.cnt, core.dPairOff, the rows' totals
int ka_ens::count_table_block(const KaEnsArgs& a, int b0, int b1, const Pass& count, std::vector<long long>& rowTot, std::vector<int>* pairCnt, double* countMs)
{
        KaEnsFamArgs f = block_args(b0, b1);
        return core.count_block("ka_ens", f, 1, [&](const KaEnsFamArgs& g) {
                KaEnsArgs x = a;
                x.i0 = b0; x.i1 = b1; x.cnt = g.cnt;
                count(x);
        }, rowTot, pairCnt, countMs);
}

// One pass of the table kernels over all rows i of a per-pair list (candidates of a level, or table entries), block by block:
// count, cut into chunks, hand over.  consume(i0, i1, b0, items, n) takes the rows i0 .. i1 of a chunk (b0: first row of the count
// block, for pairCnt -- the block's counts on the host, when asked for).
int ka_ens::stream_rows(const KaEnsArgs& a, const Pass& count, const Pass& write, const Consume& consume, std::vector<int>* pairCnt, double* countMs, double* writeMs, double* waitMs, double* chunks, long long* total)
{
        const int N = q.N, rb = count_rows();
        std::vector<long long> rowTot, rowBase;
        for (int b0 = 0; b0 < N; b0 += rb) {
                const int b1 = std::min(N, b0 + rb);
                if (count_table_block(a, b0, b1, count, rowTot, pairCnt, countMs)) return KA_FAIL;
                std::vector<KaEnsChunk> cut;
                rowBase.assign((size_t)(b1 - b0), 0);
                cut_rows(a.level, b0, b1, rowTot.data(), rowBase.data(), cut, total);
                if (core.put_row_base("ka_ens: out of device memory", rowBase)) return KA_FAIL;
                const int rc = core.hand_over("ka_ens", cut, [&](const KaEnsChunk& c, int2* out) {
                        KaEnsArgs w = a;
                        w.i0 = c.u0; w.i1 = c.u1;
                        w.pairOff = core.dPairOff.p + (long long)(c.u0 - b0) * N;
                        w.rowBase = core.dRowBase.p + (c.u0 - b0); w.out = out; w.entOut = reinterpret_cast<uint2*>(out);
                        write(w);
                }, [&](const KaEnsChunk& c, const int2* p) { return consume(c.u0, c.u1, b0, p, c.total); }, writeMs, waitMs, chunks);
                if (rc) return rc;
        }
        return KA_OK;
}

int ka_ens::consensus(int minSup, const uint8_t* letters)
{
        using clk = std::chrono::steady_clock;
        const int T = q.T, N = q.N;
        const std::vector<int>& lens = q.lens;
        const std::vector<int>& offs = q.offs;
        st[2] = st[3] = st[4] = st[5] = st[7] = st[8] = st[9] = 0.0;
        std::fill_n(levelCount, KA_ENS_MAX_RUNS + 1, 0LL);
        std::fill_n(levelMs, KA_ENS_MAX_RUNS + 1, 0.0);
        if (ensure_maps()) return KA_FAIL;
        Uf uf;
        uf.init(offs, lens, T);
        const int lo = std::max(minSup, 1), nLev = R - lo + 1, rb = count_rows();
        auto join = [&](const int2* p, long long n) {
                const auto t1 = clk::now();
                for (long long x = 0; x < n; x++) uf.join(p[x].x, p[x].y);
                st[4] += ka_ens_ms_since(t1);
                return KA_OK;
        };
        hipStream_t s = core.stream;
        if (fromTable) {
                // the table's entries with popcount == level: counted and written level by level
                KaEnsArgs a = args();
                for (int L = R; L >= lo; L--) {
                        a.level = L;
                        double cms = 0.0, wms = 0.0;
                        const int rc = stream_rows(a, [s](const KaEnsArgs& x) { ka_poar_launch_level(KA_ENS_COUNT, x, s); },
                                                   [s](const KaEnsArgs& x) { ka_poar_launch_level(KA_ENS_WRITE, x, s); },
                                                   [&](int, int, int, const int2* p, long long n) { return join(p, n); }, nullptr, &cms, &wms, &st[7], &st[8],
                                                   &levelCount[L]);
                        if (rc) return rc;
                        st[2] += cms; st[3] += wms; levelMs[L] += cms + wms;
                }
        } else if (nLev > 0) {
                // the walk counts every level of a block of rows in one pass; with one block (any N up to 4096) that is one count pass
                // in all, with more the block is counted again for each level (the levels go highest first over ALL rows)
                core.fams[0].minSup = lo;
                HIPCHK(hipMemcpyAsync(core.dFams.p, core.fams.data(), sizeof(KaEnsFam), hipMemcpyHostToDevice, s));
                std::vector<long long> rowTot, rowBase;
                std::vector<std::vector<KaEnsChunk>> cut((size_t)nLev);     // of the counted block, per level
                std::vector<long long> levTot((size_t)nLev);
                KaEnsFamArgs f{};
                for (int L = R; L >= lo; L--)
                        for (int b0 = 0; b0 < N; b0 += rb) {
                                const int b1 = std::min(N, b0 + rb), rows = b1 - b0;
                                if (L == R || rb < N) {
                                        f = block_args(b0, b1);
                                        if (core.count_block("ka_ens", f, nLev, [&](const KaEnsFamArgs& g) { ka_ens_launch_walk(KA_ENS_COUNT, g, rows * core.fams[0].nJC, core.ldsCand, s); },
                                                             rowTot, nullptr, &st[2]))
                                                return KA_FAIL;
                                        rowBase.assign(rowTot.size(), 0);
                                        for (int lv = 0; lv < nLev; lv++) {
                                                cut[lv].clear();
                                                levTot[lv] = 0;
                                                cut_rows(R - lv, b0, b1, rowTot.data() + (size_t)lv * rows, rowBase.data() + (size_t)lv * rows, cut[lv], &levTot[lv]);
                                        }
                                        if (core.put_row_base("ka_ens: out of device memory", rowBase)) return KA_FAIL;
                                        f.rowBase = core.dRowBase.p;
                                }
                                double wms = 0.0;
                                levelCount[L] += levTot[R - L];
                                const int rc = core.hand_over("ka_ens", cut[R - L], [&](const KaEnsChunk& c, int2* out) {
                                        KaEnsFamArgs w = f;
                                        w.blk0 = c.blk0; w.level = c.level; w.out = out;
                                        ka_ens_launch_walk(KA_ENS_WRITE, w, c.nBlk, core.ldsCand, s);
                                }, [&](const KaEnsChunk& c, const int2* p) { return join(p, c.total); }, &wms, &st[7], &st[8]);
                                if (rc) return rc;
                                st[3] += wms; levelMs[L] += wms;
                        }
        }
        st[9] = (double)uf.truncations;
        // columns numbered by first residue, ordered, filled
        const auto tt = clk::now();
        int nCols = 0;
        ka_ens_fill(uf, offs, lens, T, letters, cacheRows, &nCols);
        st[5] = ka_ens_ms_since(tt);
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
                const KaEnsArgs a = args();
                const int N = q.N, rb = count_rows();
                hipStream_t s = core.stream;
                std::vector<long long> rowTot;
                long long total = 0;
                double ms = 0.0;
                for (int b0 = 0; b0 < N; b0 += rb) {
                        const int b1 = std::min(N, b0 + rb);
                        if (count_table_block(a, b0, b1, [s](const KaEnsArgs& x) { ka_poar_launch_table(KA_ENS_COUNT, x, s); }, rowTot, nullptr, &ms)) return KA_FAIL;
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
        hipStream_t stream = core.stream;
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
                        tab[2] += ka_ens_ms_since(t0);
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
        if (open("ka_ens_open_table", runs)) return KA_FAIL;
        hipStream_t stream = core.stream;
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
        tab[2] = ka_ens_ms_since(t0);
        tab[3] = (double)tabEntries;
        return KA_OK;
}

// rows b0 .. b1 as count_rows left them (dPairOff, rowTot): the first entry of each of their pairs into pairStart, where *run
// entries lie before row b0; the rows' own first entries stay in core.dRowBase, and *run moves on to row b1
int ka_ens::pair_starts(int b0, int b1, const std::vector<long long>& rowTot, long long* run, long long* pairStart)
{
        std::vector<long long> base((size_t)(b1 - b0));
        for (int i = b0; i < b1; i++) { base[i - b0] = *run; *run += rowTot[i - b0]; }
        if (core.put_row_base("ka_ens: out of device memory", base)) return KA_FAIL;
        ka_poar_launch_pair_start(core.dPairOff.p, core.dRowBase.p, b0, b1, q.N, pairStart, core.stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(core.stream));
        return KA_OK;
}

// the handle's table where a kernel can read it: a table-backed handle's own; the members' table built into ps / ent in full
// (the table passes of table_emit, without the chunked hand-over to the host)
int ka_ens::table_on_device(DevBuf<long long>& ps, DevBuf<uint2>& ent, TabRef* t)
{
        if (fromTable) { *t = TabRef{ dPairStart.p, dEnt.p, tabEntries }; return KA_OK; }
        long long total = 0;
        if (table_count(&total)) return KA_FAIL;
        const int N = q.N, rb = count_rows();
        hipStream_t stream = core.stream;
        const long long nPairs = (long long)N * (N - 1) / 2;
        if (ps.alloc((size_t)nPairs + 1) || ent.alloc((size_t)std::max(total, 1LL)))
                return fail("ka_ens: out of device memory (the table of a member-backed operand, " + std::to_string(total) + " entries)");
        const KaEnsArgs a = args();
        std::vector<long long> rowTot;
        long long run = 0;
        double ms = 0.0;
        for (int b0 = 0; b0 < N; b0 += rb) {
                const int b1 = std::min(N, b0 + rb);
                if (count_table_block(a, b0, b1, [stream](const KaEnsArgs& x) { ka_poar_launch_table(KA_ENS_COUNT, x, stream); }, rowTot, nullptr, &ms)) return KA_FAIL;
                if (pair_starts(b0, b1, rowTot, &run, ps.p)) return KA_FAIL;
                KaEnsArgs w = a;
                w.i0 = b0; w.i1 = b1;
                w.pairOff = core.dPairOff.p; w.rowBase = core.dRowBase.p; w.entOut = ent.p;
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
int ka_ens::derive_table(const char* who, KaEnsArgs a, const std::function<void(int, const KaEnsArgs&)>& launch)
{
        const int N = q.N, rb = count_rows();
        hipStream_t stream = core.stream;
        const long long nPairs = (long long)N * (N - 1) / 2;
        if (dPairStart.alloc((size_t)nPairs + 1)) return fail(std::string(who) + ": out of device memory (the table)");
        std::fill_n(tab, KA_ENS_TABLE_STATS, 0.0);
        std::vector<long long> rowTot;
        long long run = 0;
        for (int b0 = 0; b0 < N; b0 += rb) {
                const int b1 = std::min(N, b0 + rb);
                if (count_table_block(a, b0, b1, [&](const KaEnsArgs& x) { launch(KA_ENS_COUNT, x); }, rowTot, nullptr, &tab[0])) return KA_FAIL;
                if (pair_starts(b0, b1, rowTot, &run, dPairStart.p)) return KA_FAIL;
        }
        if (dEnt.alloc((size_t)std::max(run, 1LL))) return fail(std::string(who) + ": out of device memory (the table, " + std::to_string(run) + " entries)");
        HIPCHK(hipMemcpyAsync(dPairStart.p + nPairs, &run, sizeof(long long), hipMemcpyHostToDevice, stream));
        a.i0 = 0; a.i1 = N;
        a.outStart = dPairStart.p; a.entOut = dEnt.p;
        HIPCHK(hipEventRecord(core.ev0, stream));
        launch(KA_ENS_WRITE, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(core.ev1, stream));
        HIPCHK(hipStreamSynchronize(stream));
        tab[1] = core.evMs();
        tabEntries = run;
        tab[3] = (double)run;
        return KA_OK;
}

// a handle for these sequences, without a source of support yet (ka_ens::open follows once n_runs is known)
static int ens_new(const char* who, ka_ctx* ctx, int numseq, const int* lens, std::unique_ptr<ka_ens>& e)
{
        e.reset(new ka_ens);
        e->ctx = ctx;
        int device = 0;
        hipStream_t stream = nullptr;
        if (ka_ctx_device_stream(ctx, &device, &stream)) return fail(std::string(who) + ": bad context");
        return e->q.set(who, numseq, lens, KA_ENS_MAX_RES, "residue indices must stay below 4096 (the reference's POAR key ri << 20 | rj aliases beyond)");
}

extern "C" int ka_ens_create(ka_ctx* ctx, int numseq, const int* lens, int n_runs, ka_ens** out)
{
        if (!ctx || !out || numseq < 1 || !lens) return fail("ka_ens_create: bad arguments");
        if (n_runs < 1 || n_runs > KA_ENS_MAX_RUNS)
                return fail("ka_ens_create: n_runs " + std::to_string(n_runs) + " outside 1.." + std::to_string(KA_ENS_MAX_RUNS) + " (one bit per member in the reference's POAR table)");
        *out = nullptr;
        std::unique_ptr<ka_ens> e;
        if (ens_new("ka_ens_create", ctx, numseq, lens, e) || e->open("ka_ens_create", n_runs)) return KA_FAIL;
        *out = e.release();
        return KA_OK;
}

extern "C" void ka_ens_destroy(ka_ens* e)
{
        if (!e) return;
        e->core.close();
        delete e;
}

extern "C" int ka_ens_add_member(ka_ens* e, int k, const uint8_t* rows, long long row_stride, int alnlen)
{
        if (e && e->fromTable) return fail("ka_ens_add_member: this handle was opened from a POAR table and takes no members");
        if (!e || k < 0 || k >= e->R) return fail("ka_ens_add_member: bad arguments");
        if (ka_msa_check_rows("ka_ens_add_member", e->q, rows, row_stride, alnlen)) return KA_FAIL;
        if (e->core.member_fits("ka_ens_add_member", k, &alnlen)) return KA_FAIL;
        HIPCHK(hipSetDevice(e->core.device));
        if (e->core.dRows[k].alloc((size_t)e->q.N * alnlen)) return fail("ka_ens_add_member: out of device memory");
        if (ka_msa_upload_rows(e->q, e->core.dRows[k].p, rows, row_stride, alnlen, e->core.stream)) return KA_FAIL;
        if (e->core.member_added(k, &alnlen)) return KA_FAIL;
        HIPCHK(hipStreamSynchronize(e->core.stream));
        e->generation++;
        return KA_OK;
}

extern "C" int ka_ens_score_rows(ka_ens* e, const uint8_t* rows, long long row_stride, int alnlen, long long* sum_out, double* score_out)
{
        if (!e) return fail("ka_ens_score_rows: bad arguments");
        if (ka_msa_check_rows("ka_ens_score_rows", e->q, rows, row_stride, alnlen)) return KA_FAIL;
        HIPCHK(hipSetDevice(e->core.device));
        if (e->ensure_maps()) return KA_FAIL;
        const KaEnsSupport table = e->lookup(KA_ENS_SCORE, alnlen);
        const int rc = e->core.score_x("ka_ens_score_rows", &alnlen, e->upload(rows, row_stride, alnlen), e->fromTable ? &table : nullptr, sum_out, score_out);
        e->st[1] = e->core.scoreMs;
        return rc;
}

extern "C" int ka_ens_consensus(ka_ens* e, int min_support, const uint8_t* letters, uint8_t* rows_out, long long row_stride, int* alnlen_out)
{
        if (!e || !letters || min_support < 1) return fail("ka_ens_consensus: bad arguments (min_support >= 1, letters)");
        HIPCHK(hipSetDevice(e->core.device));
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
        HIPCHK(hipSetDevice(e->core.device));
        if (e->ensure_maps()) return KA_FAIL;
        const KaEnsSupport table = e->lookup(KA_ENS_CONF, alnlen);
        const int rc = e->core.confidence("ka_ens_confidence", &alnlen, e->upload(rows, row_stride, alnlen), e->fromTable ? &table : nullptr, res_conf_out, col_conf_out);
        e->st[6] = e->core.confMs;
        return rc;
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
        HIPCHK(hipSetDevice(e->core.device));
        long long n = 0;
        if (e->table_count(&n)) return KA_FAIL;
        if (bytes_out) *bytes_out = 16 + 4 * ((long long)e->q.N * (e->q.N - 1) / 2) + 8 * n;
        if (entries_out) *entries_out = n;
        return KA_OK;
}

extern "C" int ka_ens_table_write(ka_ens* e, const char* path)
{
        if (!e || !path) return fail("ka_ens_table_write: bad arguments");
        HIPCHK(hipSetDevice(e->core.device));
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
        HIPCHK(hipSetDevice(e->core.device));
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
        if (ens_new(who, like->ctx, like->q.N, like->q.lens.data(), o) || o->open(who, n_runs)) return KA_FAIL;
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
        HIPCHK(hipSetDevice(a->core.device));
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
                hipStream_t s = o->core.stream;
                rc = o->derive_table(who, x, [s](int mode, const KaEnsArgs& y) { ka_poar_launch_merge(mode, y, s); });
        }
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
        HIPCHK(hipSetDevice(e->core.device));
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
                hipStream_t s = o->core.stream;
                rc = o->derive_table(who, x, [s](int mode, const KaEnsArgs& y) { ka_poar_launch_select(mode, y, s); });
        }
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
